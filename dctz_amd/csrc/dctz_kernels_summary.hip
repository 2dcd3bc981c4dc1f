// dctz_kernels_summary.hip -- per-tile summaries of the reconstruction, and of its error against an original, without
// writing the reconstruction (include/dctz_hip.h: dctzhip_tile_summary_t).
//
// One record of eight doubles per stream tile (4096 elements): min / max / sum / sum of squares of the elements r that
// dctzhip_decompress would write, and -- with the original x at hand (REF) -- min / max of x, max |x - r| and the sum of
// (x - r)^2, difference and square taken in the data type as k_psnr takes them.
//
// k_tile_summary: one wave per stream tile, lane b = block b, grid-stride over the tiles.  The head of a tile
// (summary_tile_values in dctz_summary_head.h, which the correction list's kernels call too) is
// ra_tile_image's: sixteen dwords of bin ids, DC, the wave scan of the flag counts, the index check (a tile that fails
// reads no AC_exact), the tile's exact coefficients staged in LDS; then dequantise_positional, block_inv and the de-scale
// multiply -- the decoders' own functions in their order, so every r is bit for bit the element the decoders write.
// The lane reduces its 64 registers (four running sums over j mod 4, joined as (0 + 1) + (2 + 3)), the wave joins the lanes
// in a butterfly: the order depends on nothing but the tile.  Lanes 0-7 store the record as one 64-byte row.
//   REF = false   LDS holds the staged coefficients only (16 KiB).
//   REF = true    a lane-per-block read of the original would stride the lanes 512 (256) bytes apart.  The original's tile
//                 comes in transposed instead, as k_compress brings its input in: LDS-DMA, whole 128-byte lines per lane
//                 group, `nt` policy, no registers, in two phases of half a block each through the 16 KiB the staged
//                 coefficients have left (TileMap's swizzled image; the lane reads its own block back with 16-byte LDS
//                 loads).  Phase 0 is issued as soon as the coefficients are consumed and lands under the inverse transform,
//                 phase 1 under the reduction of phase 0.  With 16 KiB a CU holds two waves per SIMD: one reduces while
//                 the other waits for its phase.
//
// k_tile_summary_rem: the short last block, decoded as k_decompress_range_rem decodes it (with k_decompress_coarse_rem's
// index check), reduced in a butterfly and merged into its tile's record behind the main kernel in stream order -- or
// written as that record when the tile holds no whole block.
// k_tile_summary_final: SUMMARY_FIN_WG records -> one, a thread per record, butterfly, then the waves in order.  The host
// launches it level by level until one record is left: the order of the total's sums depends on the tile count alone.
#include "dctz_summary_head.h"

namespace dctz {

// A lane's elements [J0, J1) of its block into its record: four running sums over j mod 4 (joined by the caller as
// (0 + 1) + (2 + 3)); with REF against the same elements of the original in o[]
template <typename T, bool REF, int J0, int J1>
__device__ __forceinline__ void summary_reduce(SumRec& a, double (&s)[4], double (&q)[4], double (&eq)[4], const T (&x)[64], const T (&o)[64]) {
#pragma unroll
  for (int j = J0; j < J1; j++) {
    const double d = (double)x[j];
    a.v[0] = fmin(a.v[0], d); a.v[1] = fmax(a.v[1], d);
    s[j & 3] = s[j & 3] + d;
    q[j & 3] = q[j & 3] + d * d;
    if constexpr (REF) {
      const double dx = (double)o[j];
      const T er = o[j] - x[j];                                        // util.c:72-73 / :88-89: difference and square in the data type
      a.v[4] = fmin(a.v[4], dx); a.v[5] = fmax(a.v[5], dx);
      a.v[6] = fmax(a.v[6], (double)fabs(er));
      eq[j & 3] = eq[j & 3] + (double)(er * er);
    }
  }
}

template <typename T, int MODE, bool REF>
__global__ __launch_bounds__(64) void k_tile_summary(SummaryParams<T> p) {
  constexpr int PH = SummaryLds<T>::PH;
  using G = Geo<T, PH>;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[SummaryLds<T>::BYTES];
  float* const stage = reinterpret_cast<float*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  TileMap<T, PH> tm;
  if (REF) tm.init(lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_decompress_range)
    asm volatile("" ::: "memory");
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned nblk = min(b0 + (unsigned)TILE_BLKS, p.nfull) - b0;   // the tile's whole blocks
    const bool full = (unsigned)lane < nblk;
    // the original's blocks of this tile; the range check zero-fills what lies beyond the last whole block
    const __amdgpu_buffer_rsrc_t r_ref =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(REF ? p.ref + (size_t)t * TILE_ELEMS : nullptr), 0, REF ? (int)(nblk * (unsigned)G::BLKB) : 0, 0x00020000);
    T x[64], o[64];
    // behind the second barrier of summary_tile_values the staged coefficients are consumed: phase 0 of the original is on
    // its way into the same LDS while the block is transformed
    if (!summary_tile_values<T, MODE>(p, t, lane, tab, qtl, scale, stage, x, [&] {
          if constexpr (REF) issue_phase_dma<T, PH>(r_ref, 0u, 0, lds, tm);
        })) { bad = true; continue; }
    SumRec a;
    a.init();
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0}, eq[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (REF) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // phase 0 has landed (and everything older is done)
      read_phase<T, PH, 0>(o, lds, tm);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // ... and is in registers before phase 1 overwrites it
      issue_phase_dma<T, PH>(r_ref, 0u, 1, lds, tm);
      if (full) summary_reduce<T, REF, 0, 32>(a, s, q, eq, x, o);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      read_phase<T, PH, 1>(o, lds, tm);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // ... before the next tile's staging writes the buffer
      if (full) summary_reduce<T, REF, 32, 64>(a, s, q, eq, x, o);
    } else {
      if (full) summary_reduce<T, REF, 0, 64>(a, s, q, eq, x, o);
    }
    a.v[2] = (s[0] + s[1]) + (s[2] + s[3]);
    a.v[3] = (q[0] + q[1]) + (q[2] + q[3]);
    if constexpr (REF) a.v[7] = (eq[0] + eq[1]) + (eq[2] + eq[3]);
    sum_wave<REF ? 8 : 4>(a);
    if constexpr (!REF) { a.v[4] = 0.0; a.v[5] = 0.0; }                // no original: the four fields are zero
    const double v = sum_field_of_lane(a, lane);
    if (lane < 8) reinterpret_cast<double*>(p.recs + t)[lane] = v;
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The short last block (length l = n % 64), one wave, lane k = element k
template <typename T, int MODE, bool REF>
__global__ __launch_bounds__(64) void k_tile_summary_rem(SummaryParams<T> p) {
  __shared__ T a[64], cr[128], ci[128];
  const int k = threadIdx.x;
  const int l = (int)(p.n - p.nfull * 64u);
  const size_t base = (size_t)p.nfull * 64;
  const unsigned t = p.nfull / (unsigned)TILE_BLKS;                    // the tile that holds the short block
  T val;
  if (!summary_rem_value<T, MODE>(p, k, a, cr, ci, val)) return;       // (wave-uniform) refused, nothing of AC_exact read
  SumRec s;
  s.init();
  if (k < l) {
    const double d = (double)val;
    s.v[0] = fmin(s.v[0], d); s.v[1] = fmax(s.v[1], d); s.v[2] = d; s.v[3] = d * d;
    if constexpr (REF) {
      const T o = p.ref[base + (size_t)k];
      const T er = o - val;
      const double dx = (double)o;
      s.v[4] = fmin(s.v[4], dx); s.v[5] = fmax(s.v[5], dx);
      s.v[6] = fmax(s.v[6], (double)fabs(er));
      s.v[7] = (double)(er * er);
    }
  }
  sum_wave<REF ? 8 : 4>(s);
  if constexpr (!REF) { s.v[4] = 0.0; s.v[5] = 0.0; }
  double v = sum_field_of_lane(s, k);
  if (k < 8) {
    double* const rec = reinterpret_cast<double*>(p.recs + t);
    // whole blocks in the tile: their record is the main kernel's, written in front of this launch in stream order
    if ((p.nfull % (unsigned)TILE_BLKS) != 0u && (REF || k < 4)) {
      const double old = rec[k];
      v = (k == 0 || k == 4) ? fmin(old, v) : (k == 1 || k == 5 || k == 6) ? fmax(old, v) : old + v;
    }
    rec[k] = v;
  }
}

// Records [SUMMARY_FIN_WG b, SUMMARY_FIN_WG (b + 1)) of `in` (m in all) -> out[b]
__global__ __launch_bounds__(SUMMARY_FIN_WG) void k_tile_summary_final(const dctzhip_tile_summary_t* __restrict__ in, const unsigned m,
                                                                       dctzhip_tile_summary_t* __restrict__ out) {
  constexpr int NW = SUMMARY_FIN_WG / 64;
  __shared__ double sh[8][NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned i = blockIdx.x * (unsigned)SUMMARY_FIN_WG + threadIdx.x;
  SumRec a;
  a.init();
  if (i < m) {
    const double* const r = reinterpret_cast<const double*>(in + i);
#pragma unroll
    for (int f = 0; f < 8; f++) a.v[f] = r[f];
  }
  sum_wave<8>(a);
  const double v = sum_field_of_lane(a, lane);
  if (lane < 8) sh[lane][wave] = v;
  __syncthreads();
  if (threadIdx.x < 8) {
    const int f = threadIdx.x;
    double acc = sh[f][0];
    for (int w = 1; w < NW; w++) acc = (f == 0 || f == 4) ? fmin(acc, sh[f][w]) : (f == 1 || f == 5 || f == 6) ? fmax(acc, sh[f][w]) : acc + sh[f][w];
    reinterpret_cast<double*>(out + blockIdx.x)[f] = acc;
  }
}

// The instantiation of (mode, with an original)
template <typename T>
auto summary_kernel(int mode, bool ref) -> void (*)(SummaryParams<T>) {
  using Fn = void (*)(SummaryParams<T>);
  return with_mode_bool(mode, ref, [](auto M, auto R) -> Fn { return k_tile_summary<T, M(), R()>; });
}
template <typename T>
int summary_occupancy(int mode, bool ref) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)summary_kernel<T>(mode, ref), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_tile_summary(const SummaryParams<T>& p, int mode, bool ref, int grid, bool with_rem, hipStream_t s) {
  using Fn = void (*)(SummaryParams<T>);
  if (grid > 0) hipLaunchKernelGGL(summary_kernel<T>(mode, ref), dim3(grid), dim3(64), 0, s, p);
  if (with_rem)
    hipLaunchKernelGGL(with_mode_bool(mode, ref, [](auto M, auto R) -> Fn { return k_tile_summary_rem<T, M(), R()>; }), dim3(1), dim3(64), 0, s, p);
}
size_t summary_final_slots(size_t m) {
  size_t slots = 0;
  do { m = (m + SUMMARY_FIN_WG - 1) / SUMMARY_FIN_WG; slots += m; } while (m > 1);
  return slots;
}
const dctzhip_tile_summary_t* launch_tile_summary_final(const dctzhip_tile_summary_t* recs, size_t m, dctzhip_tile_summary_t* part, hipStream_t s) {
  do {
    const size_t g = (m + SUMMARY_FIN_WG - 1) / SUMMARY_FIN_WG;
    hipLaunchKernelGGL(k_tile_summary_final, dim3((unsigned)g), dim3(SUMMARY_FIN_WG), 0, s, recs, (unsigned)m, part);
    recs = part; part += g; m = g;
  } while (m > 1);
  return recs;
}
template int summary_occupancy<double>(int, bool);
template int summary_occupancy<float>(int, bool);
template void launch_tile_summary<double>(const SummaryParams<double>&, int, bool, int, bool, hipStream_t);
template void launch_tile_summary<float>(const SummaryParams<float>&, int, bool, int, bool, hipStream_t);

}  // namespace dctz
