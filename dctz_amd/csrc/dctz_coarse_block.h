// dctz_coarse_block.h -- what the coarse decoders share per stream tile and per block (dctz_kernels_coarse.hip: the whole
// array; dctz_kernels_ndcbox.hip: a box of a tiled array in coarse coordinates): which of a block's 64 positions are kept,
// the head of a tile -- bin ids, DC, the wave scan of the flag counts, the index check -- and the de-quantise step of the
// kept positions.  One text for both translation units: the box decoder's values are the whole-array decoder's, bit for bit.
#pragma once

#include "dctz_kernel_common.h"

namespace dctz {

// Where position j of a block's 64 goes in the lane's array of kept coefficients (row-major low corner), or -1
template <int GEOM, int K>
__host__ __device__ constexpr int coarse_slot(int j) {
  if (GEOM == GEOM_1D) return j < K ? j : -1;
  if (GEOM == GEOM_2D) return ((j >> 3) < K && (j & 7) < K) ? (j >> 3) * K + (j & 7) : -1;
  return ((j >> 4) < K && ((j >> 2) & 3) < K && (j & 3) < K) ? ((j >> 4) * K + ((j >> 2) & 3)) * K + (j & 3) : -1;
}
// ... and one past the last kept position
template <int GEOM, int K>
__host__ __device__ constexpr int coarse_jend() {
  return GEOM == GEOM_1D ? K : GEOM == GEOM_2D ? 8 * (K - 1) + K : 16 * (K - 1) + 4 * (K - 1) + K;
}
template <int GEOM, int K> struct CoarseKept {
  static constexpr int N = GEOM == GEOM_1D ? K : GEOM == GEOM_2D ? K * K : K * K * K;
};

// Head of a tile (ra_tile_image's, without the staging): this lane's bin ids and DC, the wave scan of the flag counts, the
// index check.  False: the index disagrees with the tile's flags or leaves AC_exact.  True: `first` is the place of this
// block's first exact coefficient in the tile's piece, which starts at AC_exact[s0].
template <typename T>
__device__ __forceinline__ bool coarse_tile_head(const CoarseParams<T>& p, const unsigned t, const int lane, unsigned (&w)[16], float& dcv,
                                                 unsigned& first, unsigned& s0) {
  const unsigned rem = p.n - p.nfull * 64u;
  const unsigned full_end = p.nfull * 64u;
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
  unsigned cnt = 0;
  dcv = 0.f;
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
    // the short block's flags count for the tile (its cells are k_decompress_coarse_rem's)
    if (blk == p.nfull && rem)
      for (unsigned j = 1; j < rem; j++) cnt += p.bin[(size_t)full_end + j] == 255u ? 1u : 0u;
  }
  cnt += block_flag_count(w);
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
  s0 = p.idx[t];
  const unsigned s1 = p.idx[t + 1];
  if (s1 < s0 || s1 - s0 != tot || s1 > p.ac_count) return false;
  first = incl - cnt;
  return true;
}

// The kept positions of one block, de-quantised as dequantise_positional does it (dctz-decomp-lib.c:389-417 / :438-463):
// (T)DC, the bin centre, or the exact value with qt_restore in QT mode.  `ac` is the tile's piece of AC_exact, `ptr` this
// block's first place in it; the flags of the positions passed over advance it.  A whole block's reads stay inside the
// piece: the index check has run.
template <typename T, int MODE, int GEOM, int K, int NK>
__device__ __forceinline__ void coarse_dequantise(T (&c)[NK], const unsigned (&w)[16], const float dcv, const float* ac,
                                                  unsigned ptr, const QtLanes<T>& qtl, const CoarseParams<T>& p) {
  static_assert(NK == CoarseKept<GEOM, K>::N, "one slot per kept position");
  const BinCentres<T, true> centre{p.bin_width, nullptr};
#pragma unroll
  for (int j = 0; j < coarse_jend<GEOM, K>(); j++) {
    const int g = j >> 2, i = j & 3;
    const int sl = coarse_slot<GEOM, K>(j);
    const bool fl = j != 0 && ((w[g] >> (8 * i)) & 255u) == 255u;      // :400 / :446 (j = 0 is the DC slot, :392 / :438)
    if (sl >= 0) {
      T v;
      if (j == 0) {
        v = (T)dcv;
      } else {
        v = centre.at(bin_dword(w[g]), i);
        if (fl) {
          v = (T)ac[ptr];
          if (MODE == DCTZHIP_QT) v = qt_restore(v, qtl.at(j), p.eb, T(10), p.range_min, p.range_max);
        }
      }
      c[sl] = v;
    }
    ptr += fl ? 1u : 0u;
  }
}

}  // namespace dctz
