// dctz_summary_head.h -- the head of a stream tile that the tile summaries (dctz_kernels_summary.hip) and the correction
// list (dctz_kernels_fixup.hip) share: one wave up to the 64 elements per lane that the decoders would write, and the LDS
// such a wave needs when the original's tile follows the staged coefficients through the same buffer.  The record of eight
// doubles in a lane's registers and its join over the wave are here as well: the flat summaries and those of a tiled array
// (dctz_kernels_ndsummary.hip) write the same record.
#pragma once

#include "dctz_kernel_common.h"

namespace dctz {

constexpr double SUM_HUGE = 1.79769313486231570815e308;                // k_psnr's starting pair: min = +SUM_HUGE, max = -SUM_HUGE

// The eight fields of a record in a lane's registers
struct SumRec {
  double v[8];                                                         // rmin, rmax, rsum, rsq, xmin, xmax, emax, esq
  __device__ __forceinline__ void init() {
    v[0] = SUM_HUGE; v[1] = -SUM_HUGE; v[2] = 0.0; v[3] = 0.0; v[4] = SUM_HUGE; v[5] = -SUM_HUGE; v[6] = 0.0; v[7] = 0.0;
  }
};
// field f joins as a minimum (0, 4), a maximum (1, 5, 6) or a sum (2, 3, 7); a NaN is passed over by the first two
__device__ __forceinline__ double sum_join(const int f, const double a, const double b) {
  return (f == 0 || f == 4) ? fmin(a, b) : (f == 1 || f == 5 || f == 6) ? fmax(a, b) : a + b;
}
// ... over the wave: every lane ends with the same eight values (a butterfly; the partners' operands commute)
template <int NF>
__device__ __forceinline__ void sum_wave(SumRec& a) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int f = 0; f < NF; f++) a.v[f] = sum_join(f, a.v[f], __shfl_xor(a.v[f], d));
  }
}
// lanes 0-7 hold field `lane` of the wave's record
__device__ __forceinline__ double sum_field_of_lane(const SumRec& a, const int lane) {
  double v = a.v[0];
#pragma unroll
  for (int f = 1; f < 8; f++) {
    v = lane == f ? a.v[f] : v;
    asm volatile("" : "+v"(v));                                        // seven selects, not a table in scratch memory indexed by the lane
  }
  return v;
}

// Tile t by one wave up to the lane's 64 reconstructed elements in registers: ra_tile_image without the image.  `stage`
// holds a dense tile's exact coefficients (63 * 64 floats).  False: the index disagrees with the tile's own flags or leaves
// the caller's AC_exact; nothing of AC_exact was read.  stage_free() runs once the staged coefficients are consumed, in front
// of the transform: `stage` is the caller's again.
template <typename T, int MODE, typename F>
__device__ __forceinline__ bool summary_tile_values(const SummaryParams<T>& p, const unsigned t, const int lane, const CTab<T> tab,
                                                    const QtLanes<T>& qtl, const bool scale, float* const stage, T (&x)[64], F&& stage_free) {
  const unsigned rem = p.n - p.nfull * 64u;
  const unsigned full_end = p.nfull * 64u;
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
  unsigned w[16];
  float dcv = 0.f;
  unsigned cnt = 0;
  if (blk < p.nfull) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    dcv = p.dc[blk];
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0u;
    // the short block's flags count for the tile (its elements are k_tile_summary_rem's)
    if (blk == p.nfull && rem)
      for (unsigned j = 1; j < rem; j++) cnt += p.bin[(size_t)full_end + j] == 255u ? 1u : 0u;
  }
  cnt += block_flag_count(w);
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
  const unsigned s0 = p.idx[t], s1 = p.idx[t + 1];
  if (s1 < s0 || s1 - s0 != tot || s1 > p.ac_count) return false;
  for (unsigned i = (unsigned)lane; i < tot; i += 64u) stage[i] = p.ac[s0 + i];
  __syncthreads();
  unsigned ptr = incl - cnt;                                           // this block's first exact coefficient in the tile
  dequantise_positional<T, MODE, false>(x, w, dcv, ptr, stage, (unsigned)(63 * 64 - 1), BinCentres<T, true>{p.bin_width, nullptr},
                                        [&](int j) { return qtl.at(j); }, p.eb, p.range_min, p.range_max);
  __syncthreads();                                                     // the staged coefficients are consumed
  stage_free();
  block_inv<T, CTab<T>, GEOM_1D, (sizeof(T) == 4)>(x, tab);
  if (scale) {
#pragma unroll
    for (int j = 0; j < 64; j++) x[j] = x[j] * p.sf;                   // dctz-decomp-lib.c:494-511
  }
  return true;
}

// summary_tile_values for a stream tile of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (GEOM): the lane's block comes out of
// block_inv<GEOM>, x[j] is in-block place j (row-major in the brick).  Such streams hold whole blocks only (n = 64 nfull), so
// the short block's branch is gone; a lane beyond the last block decodes zeros that its caller masks out.  P: NdSummaryParams<T>.
template <typename T, int MODE, int GEOM, typename P>
__device__ __forceinline__ bool summary_tile_values_nd(const P& p, const unsigned t, const int lane, const CTab<T> tab, const QtLanes<T>& qtl,
                                                       const bool scale, float* const stage, T (&x)[64]) {
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
  unsigned w[16];
  float dcv = 0.f;
  if (blk < p.nfull) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    dcv = p.dc[blk];
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0u;
  }
  const unsigned cnt = block_flag_count(w);
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
  const unsigned s0 = p.idx[t], s1 = p.idx[t + 1];
  if (s1 < s0 || s1 - s0 != tot || s1 > p.ac_count) return false;
  for (unsigned i = (unsigned)lane; i < tot; i += 64u) stage[i] = p.ac[s0 + i];
  __syncthreads();
  unsigned ptr = incl - cnt;                                           // this block's first exact coefficient in the tile
  dequantise_positional<T, MODE, false>(x, w, dcv, ptr, stage, (unsigned)(63 * 64 - 1), BinCentres<T, true>{p.bin_width, nullptr},
                                        [&](int j) { return qtl.at(j); }, p.eb, p.range_min, p.range_max);
  __syncthreads();                                                     // the staged coefficients are consumed
  block_inv<T, CTab<T>, GEOM, (sizeof(T) == 4)>(x, tab);
  if (scale) {
#pragma unroll
    for (int j = 0; j < 64; j++) x[j] = x[j] * p.sf;                   // dctz-decomp-lib.c:494-511
  }
  return true;
}

// The short last block (length l = n % 64) by one wave, lane k = element k, as k_decompress_range_rem decodes it with
// k_decompress_coarse_rem's index check: lanes k < l leave with their element in `val`.  a: 64, cr / ci: 128 elements of LDS.
// False (wave-uniform): the index disagrees with the flags of the block's tile; error = 2 is set and nothing of AC_exact read.
template <typename T, int MODE>
__device__ __forceinline__ bool summary_rem_value(const SummaryParams<T>& p, const int k, T* a, T* cr, T* ci, T& val) {
  const int l = (int)(p.n - p.nfull * 64u);
  const size_t base = (size_t)p.nfull * 64;
  const unsigned t = p.nfull / (unsigned)TILE_BLKS;                    // the tile that holds the short block
  unsigned cfront = 0;                                                 // flags of the tile's whole blocks in front of it
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)k;
  if (blk < p.nfull) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
    unsigned w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    cfront = block_flag_count(w);
  }
  const unsigned front = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(cfront), 63);
  unsigned b = 0;
  if (k < l) b = p.bin[base + k];
  const bool exc = (k < l) && (k != 0) && (b == 255u);
  const unsigned long long msk = __ballot(exc);
  const unsigned rank = (unsigned)__popcll(msk & ((1ull << k) - 1ull));
  const unsigned s0 = p.idx[t], s1 = p.idx[t + 1];
  if (s1 < s0 || s1 - s0 != front + (unsigned)__popcll(msk) || s1 > p.ac_count) {
    if (k == 0) atomicExch(&p.ctl->error, 2u);
    return false;
  }
  const unsigned start = s0 + front;
  short_inv_clear(cr, ci, k);
  if (k < l) {
    T e = T(0);
    if (exc) e = (T)p.ac[start + rank];
    a[k] = short_inv_value<T, MODE>(b, exc, k, k == 0 ? p.dc[p.nfull] : 0.f, e, p.bin_width, [&](int j) { return p.qtab[j]; }, p.eb, p.range_min,
                                    p.range_max);
  }
  __syncthreads();
  if (k < l) short_inv_spread(cr, ci, a, p.rtab, l, k);
  __syncthreads();
  val = T(0);
  if (k < l) {
    val = short_inv_sum(cr, ci, p.rtab, l, k);
    if (p.sf != T(1)) val = val * p.sf;
  }
  return true;
}

// LDS of a wave: a dense tile's staged coefficients (63 * 64 floats), and behind them in time one phase of the original
template <typename T> struct SummaryLds {
  static constexpr int PH = 2;
  static constexpr int BYTES = Geo<T, PH>::PHB > 63 * 64 * 4 ? Geo<T, PH>::PHB : 63 * 64 * 4;
};

}  // namespace dctz
