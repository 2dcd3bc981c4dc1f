// dctz_kernels_ra.hip -- random access on decode (include/dctz_hip.h: dctzhip_ac_index, dctzhip_decompress_range).
//
// The blocks of a DCTZ stream are independent except for ONE running value: the position `pos` in AC_exact at which a
// block's exact coefficients start (dctz-decomp-lib.c:370, :402-412), the number of "stored exactly" flags in front of
// it.  The exception index gives that number every 4096 elements (a tile of 64 blocks):
//   idx[i] = flags (bin id 255 at an in-block position j with 1 <= j < block length) in elements [0, min(n, 4096 i)),
//   i = 0 .. m, m = ceil(n / 4096);  idx[m] = tot_AC_exact_count.
// k_ac_index counts the flags of 64 tiles per workgroup and scans them in one wave; k_ac_index_scan scans the workgroup
// sums in one workgroup; k_ac_index_add adds the workgroups' offsets back.
//
// k_decompress_range rebuilds elements [lo, hi) of the array from the tiles [t0, t1) that hold them: one wave per tile,
// lane b block b (the decomposition of k_decompress), the tile's exact coefficients AC_exact[idx[t], idx[t + 1]) staged
// in LDS, in-tile placement a wave scan of the blocks' flag counts.  Bin centres, QT de-quantisation, the inverse block
// transform and the de-scaling are the whole-array decoders' own functions in the same order, so every element is bit
// for bit what dctzhip_decompress writes.  The reconstructed tile goes through an LDS image (a block per row, one
// 16-byte pad per row: conflict-free both ways) and leaves in output order: 16-byte stores for the chunks of d_out the
// tile owns wholly, element stores at the range's and the tile's edges.  The short last block is
// k_decompress_range_rem's (the length-l transform of k_decompress_rem).
#include "dctz_kernel_common.h"

namespace dctz {

// ================================================================== the index ==
// Workgroup g takes tiles [64 g, 64 g + 64): wave w the tiles w, w + 4, ..., IX_TF of them in flight, 16-byte loads as
// k_count_tiles reads them.  The one 16-byte group that holds the array's last byte (n % 16 != 0) is read byte by byte:
// bytes beyond n count as 0 (no flag), and the short block's positions j >= l lie beyond n.
constexpr int IX_TF = 4;
__global__ __launch_bounds__(SWG) void k_ac_index(const uint8_t* __restrict__ bin, unsigned n, unsigned m, unsigned* __restrict__ idx,
                                                  unsigned* __restrict__ wg_sum) {
  __shared__ unsigned tcs[IX_TPW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr unsigned NW = SWG / 64;
  const unsigned first = blockIdx.x * (unsigned)IX_TPW;
  for (unsigned r0 = (unsigned)wave; r0 < (unsigned)IX_TPW; r0 += IX_TF * NW) {
    uint4 wv[IX_TF][4];
#pragma unroll
    for (int h = 0; h < IX_TF; h++) {
      const unsigned tile = first + r0 + (unsigned)h * NW;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const size_t o = (size_t)tile * TILE_ELEMS + (size_t)i * 1024 + (size_t)lane * 16;
        wv[h][i] = make_uint4(0u, 0u, 0u, 0u);
        if (tile < m && o + 16 <= (size_t)n) wv[h][i] = *reinterpret_cast<const uint4*>(bin + o);
        else if (tile < m && o < (size_t)n) {
          unsigned w[4] = {0u, 0u, 0u, 0u};
          for (unsigned b = 0; b < 16u && o + b < (size_t)n; b++) w[b >> 2] |= (unsigned)bin[o + b] << (8 * (b & 3));
          wv[h][i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
#pragma unroll
    for (int h = 0; h < IX_TF; h++) {
      unsigned c = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const unsigned w[4] = {wv[h][i].x, wv[h][i].y, wv[h][i].z, wv[h][i].w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          unsigned f = exact_flags(w[k]);
          if (k == 0 && (lane & 3) == 0) f &= ~0x80u;                    // byte 0 of every 64: j = 0, the DC slot
          c += (unsigned)__popc(f);
        }
      }
      const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(c), 63);
      if (lane == 0) tcs[r0 + (unsigned)h * NW] = tot;                 // (0 for tiles beyond m: nothing was loaded)
    }
  }
  __syncthreads();
  if (wave == 0) {
    const unsigned v = tcs[lane];
    const unsigned incl = wave_incl_scan(v);
    const unsigned tile = first + (unsigned)lane;
    if (tile < m) idx[tile] = incl - v;                                // exclusive prefix inside the workgroup's tiles
    if (lane == 63) wg_sum[blockIdx.x] = incl;
  }
}

// One workgroup: exclusive prefix of the g workgroup sums, in place; idx[m] = their total
constexpr int IX_SWG = 1024;
__global__ __launch_bounds__(IX_SWG) void k_ac_index_scan(unsigned* __restrict__ wg_sum, unsigned g, unsigned* __restrict__ idx, unsigned m) {
  __shared__ unsigned wtot[IX_SWG / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned run = 0;
  for (unsigned i0 = 0; i0 < g; i0 += IX_SWG) {
    const unsigned i = i0 + threadIdx.x;
    const unsigned v = i < g ? wg_sum[i] : 0u;
    const unsigned incl = wave_incl_scan(v);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < IX_SWG / 64; w++) {
      const unsigned t = wtot[w];
      before += w < wave ? t : 0u;
      all += t;
    }
    if (i < g) wg_sum[i] = run + before + incl - v;
    run += all;
    __syncthreads();                                                   // wtot is rewritten by the next round
  }
  if (threadIdx.x == 0) idx[m] = run;
}

__global__ __launch_bounds__(SWG) void k_ac_index_add(unsigned* __restrict__ idx, unsigned m, const unsigned* __restrict__ wg_pre) {
  const unsigned t = blockIdx.x * (unsigned)SWG + threadIdx.x;
  if (t < m) idx[t] += wg_pre[t / (unsigned)IX_TPW];
}

void launch_ac_index(const uint8_t* bin, unsigned n, unsigned* idx, unsigned* wg_sum, hipStream_t s) {
  const unsigned m = (n + TILE_ELEMS - 1) / TILE_ELEMS;
  const unsigned g = (m + IX_TPW - 1) / IX_TPW;
  hipLaunchKernelGGL(k_ac_index, dim3(g), dim3(SWG), 0, s, bin, n, m, idx, wg_sum);
  hipLaunchKernelGGL(k_ac_index_scan, dim3(1), dim3(IX_SWG), 0, s, wg_sum, g, idx, m);
  if (g > 1) hipLaunchKernelGGL(k_ac_index_add, dim3((m + SWG - 1) / SWG), dim3(SWG), 0, s, idx, m, (const unsigned*)wg_sum);
}

// ============================================================== range decode ==
// The tile itself (flags, index check, staging, de-quantisation, transform, LDS image) is ra_tile_image's
// (dctz_kernel_common.h), shared with k_decompress_box.
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_range(RangeParams<T> p) {
  using G = RaGeo<T>;
  using Vec = typename Traits<T>::Vec;
  constexpr int EPV = G::EPV;
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::BYTES];
  T* const img = reinterpret_cast<T*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const unsigned full_end = p.nfull * 64u;
  bool bad = false;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    if (!ra_tile_image<T, MODE>(p, t, lane, tab, qtl, scale, lds)) { bad = true; continue; }
    // the tile's whole-block elements inside [lo, hi) -> d_out, in output order
    const unsigned ts = t * (unsigned)TILE_ELEMS;
    const unsigned A = max(p.lo, ts), B = min(p.hi, min(ts + (unsigned)TILE_ELEMS, full_end));
    if (A < B) {
      const unsigned oa = A - p.lo, ob = B - p.lo;                     // output positions [oa, ob)
      const unsigned qf = oa / EPV, ql = (ob + EPV - 1) / EPV;         // 16-byte chunks of d_out they touch
      const unsigned base = qf * EPV;
      // (a descriptor per tile, based at the tile's first chunk -- never in front of d_out -- and ending at its last element)
      const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out + base, 0, (int)((ob - base) * sizeof(T)), 0x00020000);
      for (unsigned q0 = qf; q0 < ql; q0 += 64u) {
        const unsigned q = q0 + (unsigned)lane;
        if (q < ql) {
          T v[EPV];
          bool in[EPV];
#pragma unroll
          for (int k = 0; k < EPV; k++) {
            const unsigned o = q * EPV + (unsigned)k;
            in[k] = o >= oa && o < ob;
            const unsigned e = in[k] ? o + p.lo - ts : 0u;             // element of the tile
            v[k] = img[G::at(e)];
          }
          const int at = (int)((q - qf) * 16u);
          bool whole = true;
#pragma unroll
          for (int k = 0; k < EPV; k++) whole = whole && in[k];
          if (whole) {
            const Vec pv = Traits<T>::pack(v);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pv), r_out, at, 0, 0);
          } else {
#pragma unroll
            for (int k = 0; k < EPV; k++) {
              if (!in[k]) continue;
              if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[k]), r_out, at + 8 * k, 0, 0);
              else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[k]), r_out, at + 4 * k, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();                                                   // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The short last block (length l = n % 64) when the range reaches into it: k_decompress_rem's length-l inverse transform
// (dctz-decomp-lib.c:423-428, dct.c:144-199), its first exact coefficient = idx[t] + the flags of the tile's whole blocks.
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_range_rem(RangeParams<T> p) {
  __shared__ T a[64];
  __shared__ T cr[128];
  __shared__ T ci[128];
  const int k = threadIdx.x;
  const int l = (int)(p.n - p.nfull * 64u);
  const size_t base = (size_t)p.nfull * 64;
  const unsigned t = p.nfull / (unsigned)TILE_BLKS;                    // the tile that holds the short block
  // flags of the tile's whole blocks in front of the short block
  unsigned c = 0;
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)k;
  if (blk < p.nfull) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
    unsigned w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    c = block_flag_count(w);
  }
  const unsigned start = p.idx[t] + (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(c), 63);
  const unsigned lim = min(p.ac_count, p.idx[t + 1]);
  unsigned b = 0;
  if (k < l) b = p.bin[base + k];
  const bool exc = (k < l) && (k != 0) && (b == 255u);
  const unsigned long long msk = __ballot(exc);
  const unsigned rank = (unsigned)__popcll(msk & ((1ull << k) - 1ull));
  short_inv_clear(cr, ci, k);
  if (k < l) {
    T e = T(0);
    if (exc) { if (start + rank < lim) e = (T)p.ac[start + rank]; else atomicExch(&p.ctl->error, 2u); }
    a[k] = short_inv_value<T, MODE>(b, exc, k, k == 0 ? p.dc[p.nfull] : 0.f, e, p.bin_width, [&](int j) { return p.qtab[j]; }, p.eb, p.range_min, p.range_max);
  }
  __syncthreads();
  if (k < l) short_inv_spread(cr, ci, a, p.rtab, l, k);
  __syncthreads();
  if (k < l) {
    T val = short_inv_sum(cr, ci, p.rtab, l, k);
    if (p.sf != T(1)) val = val * p.sf;
    const size_t e = base + (size_t)k;
    if (e >= p.lo && e < p.hi) p.out[e - p.lo] = val;
  }
}

template <typename T>
auto range_kernel(int mode) -> void (*)(RangeParams<T>) {
  return with_mode(mode, [](auto M) { return k_decompress_range<T, M()>; });
}
template <typename T>
int range_occupancy(int mode) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)range_kernel<T>(mode), 64, 0);
  return e == hipSuccess ? n : 0;
}

template <typename T>
void launch_decompress_range(const RangeParams<T>& p, int mode, int grid, bool with_rem, hipStream_t s) {
  if (grid > 0) hipLaunchKernelGGL(range_kernel<T>(mode), dim3(grid), dim3(64), 0, s, p);
  if (with_rem) hipLaunchKernelGGL(with_mode(mode, [](auto M) { return k_decompress_range_rem<T, M()>; }), dim3(1), dim3(64), 0, s, p);
}
template int range_occupancy<double>(int);
template int range_occupancy<float>(int);
template void launch_decompress_range<double>(const RangeParams<double>&, int, int, bool, hipStream_t);
template void launch_decompress_range<float>(const RangeParams<float>&, int, int, bool, hipStream_t);

}  // namespace dctz
