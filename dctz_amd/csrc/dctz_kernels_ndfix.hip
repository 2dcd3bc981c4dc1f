// dctz_kernels_ndfix.hip -- the correction list of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h:
// dctzhip_fixup_build_nd / dctzhip_fixup_apply_nd).
//
// The list's positions are the streams': position q = 64 B + j, block B row-major over the block grid, j row-major inside
// the brick.  The original and the output are the array itself, so every kernel here turns stream positions into array
// coordinates; none of them sees a gathered copy.
//
// k_ndfix_mark: k_decompress_ndbox's loop over ALL stream tiles.  ra_tile_image leaves the reconstructed tile in LDS (bit
// for bit the elements dctzhip_decompress_nd writes); the tile is walked in the row strips that kernel stores -- step s,
// in-block row r: lane l holds strip element l + 64 s -- and where that kernel stores, this one compares with the original,
// loaded under the same predicate (the loads of several steps are issued together, behind the decode).  The ballot of a
// comparison holds the e bits of row r for each of the 64 / e blocks of the step; lane b, owner of block b, shifts its e
// bits to place e r of its mask when s is its step.  A padded position is never loaded and never listed.  The lane stores
// its mask (the flat family's scratch, one word per block), a wave sum of the popcounts is the tile's count.
// k_ndfix_emit: k_fixup_emit with the original fetched at the block's coordinates: the wave writes block after block, lane j
// the entry of in-block place j.
// k_ndfix_apply: k_fixup_apply over the candidate stream tiles of a box; the untrusted list is compared first -- table,
// offsets, block < nblk, no padded position -- and a tile that fails stores nothing.
// The prefix of the tiles' counts is k_fixup_scan, unchanged.
#include "dctz_nd_image.h"

namespace dctz {

template <typename T, int MODE, int GEOM>
__global__ __launch_bounds__(64) void k_ndfix_mark(NdFixParams<T> p) {
  using G = NdImage<T, GEOM>;
  constexpr unsigned E = GEOM == GEOM_2D ? 8u : 4u;                    // block edge
  constexpr int ROWS = 64 / (int)E;                                    // in-block rows of E elements
  constexpr unsigned BPS = 64u / E;                                    // blocks per step
  constexpr unsigned SB = sizeof(T) == 8 ? E / 2u : E;                 // steps whose loads of the original are in flight together
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::BYTES];
  const T* const img = reinterpret_cast<const T*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned dx = p.d[2], dy = p.d[1], dz = p.d[0];
  const T* __restrict__ const ref = p.ref;
  const unsigned my_step = (unsigned)lane / BPS;                       // the step that holds this lane's own block
  const unsigned my_shift = ((unsigned)lane % BPS) * E;                // ... and its bits in that step's ballots
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.nfull);
    if (!ra_tile_image<T, MODE, GEOM, G>(p, t, lane, tab, qtl, scale, lds)) {
      bad = true;
      if (lane == 0) p.tile_cnt[t] = 0u;
      continue;
    }
    // The original's strip elements of SB steps, SB ROWS a lane, are issued together behind the decode, when the block's
    // registers are free again: one round trip per batch instead of one per step.  fp32 takes the whole tile at once; fp64
    // half of it, because 64 loads in flight hold 128 registers of values and as many of addresses.  A position that is not
    // real is not loaded and its bit stays clear.
    unsigned long long msk = 0ull;
#pragma unroll
    for (unsigned h = 0; h < E; h += SB) {
      asm volatile("" ::: "memory");                                   // (a batch's loads stay behind the decode and behind the batch in front)
      T o[SB][ROWS];
      unsigned long long real = 0ull;                                  // bit ROWS i + r: this lane's position of step h + i, row r is real
#pragma unroll
      for (unsigned i = 0; i < SB; i++) {
        const unsigned B = b0 + (unsigned)lane / E + BPS * (h + i);    // block of the tile, in-row offset
        unsigned bz, by, bx;
        ndfix_block<GEOM>(B, nbx, nby, bz, by, bx);                    // once per lane and step
        const unsigned x = bx * E + (unsigned)lane % E;
        const bool in = B < b1 && x < dx;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          const unsigned z = GEOM == GEOM_3D ? bz * 4u + (unsigned)(r >> 2) : 0u;
          const unsigned y = GEOM == GEOM_3D ? by * 4u + (unsigned)(r & 3) : by * 8u + (unsigned)r;
          const bool ok = in && z < dz && y < dy;
          o[i][r] = T(0);
          if (ok) o[i][r] = ref[((size_t)z * dy + y) * dx + x];
          real |= (unsigned long long)ok << (i * (unsigned)ROWS + (unsigned)r);
        }
      }
#pragma unroll
      for (unsigned i = 0; i < SB; i++) {
        const T* const src = img + ((unsigned)lane / E + BPS * (h + i)) * (unsigned)G::STRIDE + (unsigned)lane % E;
        unsigned long long own = 0ull;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          const T v = src[r * (int)E];
          const bool hit = ((real >> (i * (unsigned)ROWS + (unsigned)r)) & 1ull) && !(fabs(o[i][r] - v) <= p.bound);   // a NaN on either side lists the position
          const unsigned long long bal = __ballot(hit);                // row r of the step's 64 / E blocks, E bits each
          own |= ((bal >> my_shift) & ((1ull << E) - 1ull)) << ((unsigned)r * E);
        }
        if (h + i == my_step) msk = own;
      }
    }
    if (b0 + (unsigned)lane < b1) p.mask[b0 + (unsigned)lane] = msk;   // (blocks beyond the last one never hit: msk = 0)
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan((unsigned)__popcll(msk)), 63);
    if (lane == 0) p.tile_cnt[t] = tot;
    __syncthreads();                                                   // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

template <typename T, int GEOM>
__global__ __launch_bounds__(64) void k_ndfix_emit(NdFixEmitParams<T> p) {
  const int lane = threadIdx.x;
  if (p.fix_start[p.ntiles] > p.capacity || p.ctl->error) return;      // the list does not fit, or the masks are not all there
  const T* __restrict__ const ref = p.ref;
  uint16_t* __restrict__ const fix_off = p.fix_off;
  T* __restrict__ const fix_val = p.fix_val;
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned dx = p.d[2], dy = p.d[1];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
    const unsigned long long msk = blk < p.nblk ? p.mask[blk] : 0ull;
    const unsigned c = (unsigned)__popcll(msk);
    const unsigned incl = wave_incl_scan(c);
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
    const unsigned s0 = p.fix_start[t], s1 = p.fix_start[t + 1];
    if (s1 - s0 != tot || s1 > p.capacity) continue;                   // (never, after the scan of these masks' counts)
    // Block after block by the whole wave, lane j the entry of in-block place j; the places are the scan's.  The block's grid
    // coordinates are its owner lane's, one decomposition per lane and tile.
    const unsigned at = s0 + incl - c;
    const unsigned lo = (unsigned)msk, hi = (unsigned)(msk >> 32);
    unsigned mz, my, mx;
    ndfix_block<GEOM>(blk, nbx, nby, mz, my, mx);
#pragma unroll 8
    for (int b = 0; b < TILE_BLKS; b++) {
      const unsigned long long mb = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, b) << 32) |
                                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, b);
      const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)at, b);
      const unsigned bz = (unsigned)__builtin_amdgcn_readlane((int)mz, b), by = (unsigned)__builtin_amdgcn_readlane((int)my, b),
                     bx = (unsigned)__builtin_amdgcn_readlane((int)mx, b);
      if ((mb >> lane) & 1ull) {                                       // a listed position is a real one: inside the array
        unsigned z, y, x;
        ndfix_place<GEOM>(bz, by, bx, (unsigned)lane, z, y, x);
        const unsigned i = first + (unsigned)__popcll(mb & below);
        fix_off[i] = (uint16_t)((unsigned)b * 64u + (unsigned)lane);
        fix_val[i] = ref[((size_t)z * dy + y) * dx + x];
      }
    }
  }
}

template <typename T, int GEOM>
__global__ __launch_bounds__(64) void k_ndfix_apply(NdFixApplyParams<T> p) {
  const int lane = threadIdx.x;
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned dx = p.d[2], dy = p.d[1], dz = p.d[0];
  const unsigned lox = p.lo[2], loy = p.lo[1], loz = p.lo[0];
  const unsigned ex = p.ext[2], ey = p.ext[1], ez = p.ext[0];
  bool bad = p.fix_start[p.ntiles] != p.count;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1 && !bad; t += gridDim.x) {
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned te = (min(b0 + (unsigned)TILE_BLKS, p.nblk) - b0) * 64u;   // the tile's positions
    const unsigned s0 = p.fix_start[t], s1 = p.fix_start[t + 1];
    if (s1 < s0 || s1 > p.count || s1 - s0 > te) { bad = true; break; }   // (wave-uniform) every read below stays inside [0, count)
    // every offset inside the tile's blocks, at a real position and above its neighbour in front, before anything is stored
    bool wrong = false;
    for (unsigned i = s0 + (unsigned)lane; i < s1; i += 64u) {
      const unsigned o = p.fix_off[i];
      bool w = o >= te || (i > s0 && (unsigned)p.fix_off[i - 1] >= o);
      if (!w) {
        unsigned bz, by, bx, z, y, x;
        ndfix_block<GEOM>(b0 + (o >> 6), nbx, nby, bz, by, bx);
        ndfix_place<GEOM>(bz, by, bx, o & 63u, z, y, x);
        w = z >= dz || y >= dy || x >= dx;                             // the edge padding holds no entry
      }
      wrong = wrong || w;
    }
    if (__any(wrong)) { bad = true; break; }
    for (unsigned i = s0 + (unsigned)lane; i < s1; i += 64u) {
      const unsigned o = p.fix_off[i];
      unsigned bz, by, bx, z, y, x;
      ndfix_block<GEOM>(b0 + (o >> 6), nbx, nby, bz, by, bx);
      ndfix_place<GEOM>(bz, by, bx, o & 63u, z, y, x);
      const unsigned rz = z - loz, ry = y - loy, rx = x - lox;         // box-relative; unsigned: in front of lo wraps beyond ext
      if (rz < ez && ry < ey && rx < ex) p.out[((size_t)rz * ey + ry) * ex + rx] = p.fix_val[i];
    }
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 5u);
}

// The instantiation of a mode and a geometry
template <typename T>
auto ndfix_kernel(int mode, int geom) -> void (*)(NdFixParams<T>) {
  return with_mode_bool(mode, geom == GEOM_3D, [](auto M, auto D3) { return k_ndfix_mark<T, M(), D3() ? GEOM_3D : GEOM_2D>; });
}
template <typename T>
int ndfix_occupancy(int mode, int geom) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)ndfix_kernel<T>(mode, geom), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_ndfix_mark(const NdFixParams<T>& p, int mode, int geom, int grid, hipStream_t s) {
  hipLaunchKernelGGL(ndfix_kernel<T>(mode, geom), dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
void launch_ndfix_emit(const NdFixEmitParams<T>& p, int geom, int grid, hipStream_t s) {
  if (geom == GEOM_3D) hipLaunchKernelGGL((k_ndfix_emit<T, GEOM_3D>), dim3(grid), dim3(64), 0, s, p);
  else hipLaunchKernelGGL((k_ndfix_emit<T, GEOM_2D>), dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
void launch_ndfix_apply(const NdFixApplyParams<T>& p, int geom, int grid, hipStream_t s) {
  if (geom == GEOM_3D) hipLaunchKernelGGL((k_ndfix_apply<T, GEOM_3D>), dim3(grid), dim3(64), 0, s, p);
  else hipLaunchKernelGGL((k_ndfix_apply<T, GEOM_2D>), dim3(grid), dim3(64), 0, s, p);
}
template int ndfix_occupancy<double>(int, int);
template int ndfix_occupancy<float>(int, int);
template void launch_ndfix_mark<double>(const NdFixParams<double>&, int, int, int, hipStream_t);
template void launch_ndfix_mark<float>(const NdFixParams<float>&, int, int, int, hipStream_t);
template void launch_ndfix_emit<double>(const NdFixEmitParams<double>&, int, int, hipStream_t);
template void launch_ndfix_emit<float>(const NdFixEmitParams<float>&, int, int, hipStream_t);
template void launch_ndfix_apply<double>(const NdFixApplyParams<double>&, int, int, hipStream_t);
template void launch_ndfix_apply<float>(const NdFixApplyParams<float>&, int, int, hipStream_t);

}  // namespace dctz
