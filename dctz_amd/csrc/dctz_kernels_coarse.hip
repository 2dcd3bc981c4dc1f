// dctz_kernels_coarse.hip -- the whole array at reduced resolution from the low coefficients of every block
// (include/dctz_hip.h: dctzhip_decompress_coarse, dctzhip_decompress_coarse_nd).
//
// With K = edge / factor, a block's K (flat), K x K (8 x 8 tiles) or K x K x K (4 x 4 x 4 tiles) lowest coefficients are
// de-quantised exactly as every decoder does it and go through the low-band inverse transform of dct_lowband_block.h:
//     y[i] = sf sum_{k < K} alpha_N(k) c[k] cos(pi k (2i + 1) / (2K)),
// separably along every axis of a tile.  A block writes K^d values instead of 64.
//
// One wave per stream tile of 64 blocks, lane b = block b, as in the box decoders.  A lane still loads its sixteen dwords
// of bin ids: the flags of the positions it does not de-quantise move its place in AC_exact all the same.  The wave scan
// of the flag counts places the lane in the tile's piece AC_exact[idx[t], idx[t + 1]); the index is checked against the
// tile's own flags first (ra_tile_image's check: a tile that fails reads no AC_exact).  The few exact coefficients among
// the kept positions are read straight from that piece -- staging the whole piece in LDS, as the full-resolution tile
// does, would move up to 63 / K times what is used.
//
// Stores.  Flat: the tile's 64 K outputs are contiguous in d_out; the lanes park their K values in LDS (CoarseImage: one
// element of padding behind every 32, so that the lanes' writes, K elements apart, and the read-back, consecutive across
// the lanes, both spread over the banks) and the wave stores 64 consecutive elements per instruction.  Tiles: the row
// strips of k_decompress_ndbox with K in place of the block edge -- in-block row r of all 64 blocks is a run of 64 K
// consecutive output elements up to where the tile wraps into the next block row.
//
// k_decompress_coarse_dc: factor = block edge, the DC stream alone (out[b] = sf DC[b] / 8 for every geometry: the block
// grid IS the output grid).  k_decompress_coarse_rem: the flat short block, decoded as k_decompress_range_rem decodes it,
// then the means of its cells of `factor` elements, summed left to right in the data type.
#include "dctz_coarse_block.h"
#include "dct_lowband_block.h"

namespace dctz {

// Flat blocks: the tile's 64 K outputs in LDS, element e at e + e / 32
template <typename T, int K> struct CoarseImage {
  static constexpr int ELEMS = 64 * K + 2 * K;
  __device__ static unsigned at(unsigned e) { return e + (e >> 5); }
};

template <typename T, int MODE, int K>
__global__ __launch_bounds__(64) void k_decompress_coarse(CoarseParams<T> p) {
  using G = CoarseImage<T, K>;
  __shared__ T img[G::ELEMS];
  const int lane = threadIdx.x;
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    unsigned w[16];
    float dcv;
    unsigned first, s0;
    if (!coarse_tile_head<T>(p, t, lane, w, dcv, first, s0)) { bad = true; continue; }
    T c[K], y[K];
    coarse_dequantise<T, MODE, GEOM_1D, K>(c, w, dcv, p.ac + s0, first, qtl, p);
    lowband_inv<T, 64, K>(c, y);
    if (scale) {
#pragma unroll
      for (int i = 0; i < K; i++) y[i] = y[i] * p.sf;
    }
#pragma unroll
    for (int i = 0; i < K; i++) img[G::at((unsigned)(lane * K + i))] = y[i];
    __syncthreads();
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned cnt = (min(b0 + (unsigned)TILE_BLKS, p.nfull) - b0) * (unsigned)K;    // outputs of the tile's whole blocks
    T* const out = p.out + (size_t)b0 * K;
#pragma unroll
    for (int s = 0; s < K; s++) {
      const unsigned e = (unsigned)lane + 64u * (unsigned)s;
      if (e < cnt) out[e] = img[G::at(e)];
    }
    __syncthreads();                                                   // the image is read out before the next tile writes it
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

template <typename T, int MODE, int GEOM, int K>
__global__ __launch_bounds__(64) void k_decompress_coarse_nd(CoarseParams<T> p) {
  constexpr int KD = CoarseKept<GEOM, K>::N;                            // values per block
  constexpr int ROWS = KD / K;                                         // in-block rows of K values
  constexpr int STRIDE = KD + 1;                                       // odd: the lanes' writes spread over the banks
  __shared__ T img[TILE_BLKS * STRIDE];
  const int lane = threadIdx.x;
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned odx = p.od[2], ody = p.od[1], odz = p.od[0];
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    unsigned w[16];
    float dcv;
    unsigned first, s0;
    if (!coarse_tile_head<T>(p, t, lane, w, dcv, first, s0)) { bad = true; continue; }
    T c[KD];
    coarse_dequantise<T, MODE, GEOM, K>(c, w, dcv, p.ac + s0, first, qtl, p);
    if constexpr (GEOM == GEOM_2D) lowband_inv_2d<T, K>(c); else lowband_inv_3d<T, K>(c);
    if (scale) {
#pragma unroll
      for (int i = 0; i < KD; i++) c[i] = c[i] * p.sf;
    }
#pragma unroll
    for (int i = 0; i < KD; i++) img[lane * STRIDE + i] = c[i];
    __syncthreads();
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.nfull);
#pragma unroll
    for (unsigned s = 0; s < (unsigned)K; s++) {                       // 64 K strip elements, 64 a step
      const unsigned bl = (unsigned)lane / (unsigned)K + (64u / (unsigned)K) * s;   // block of the tile, offset in its row
      const unsigned off = (unsigned)lane % (unsigned)K;
      const unsigned B = b0 + bl;
      const unsigned q = B / nbx, bx = B - q * nbx;                    // the block's grid coordinates
      const unsigned bz = GEOM == GEOM_3D ? q / nby : 0u, by = q - bz * nby;
      const unsigned ox = bx * (unsigned)K + off;
      const bool in = B < b1 && ox < odx;                              // a cell that begins past the array is not written
      const T* const src = img + bl * (unsigned)STRIDE + off;
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const T v = src[r * K];
        const unsigned oz = GEOM == GEOM_3D ? bz * (unsigned)K + (unsigned)(r / K) : 0u;
        const unsigned oy = GEOM == GEOM_3D ? by * (unsigned)K + (unsigned)(r % K) : by * (unsigned)K + (unsigned)r;
        if (in && oy < ody && oz < odz) p.out[((size_t)oz * ody + oy) * odx + ox] = v;
      }
    }
    __syncthreads();
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// factor = block edge: K = 1, y = sf c[0] / sqrt(64) for a flat block, an 8 x 8 and a 4 x 4 x 4 tile alike
template <typename T>
__global__ __launch_bounds__(SWG) void k_decompress_coarse_dc(const float* __restrict__ dc, T* __restrict__ out, const unsigned nblk, const T sf) {
  const bool scale = (sf != T(1));
  for (unsigned b = blockIdx.x * (unsigned)SWG + threadIdx.x; b < nblk; b += gridDim.x * (unsigned)SWG) {
    T v = (T)dc[b] * T(0.125);
    if (scale) v = v * sf;
    out[b] = v;
  }
}

// The flat short block (length l = n % 64), one wave: the elements dctzhip_decompress writes for it (box_rem_block's
// sequence), parked in LDS; then lane c sums cell c -- elements [c f, min(c f + f, l)) -- left to right in the data type
// and divides by the cell's element count.  The sum reads what was stored: the de-scale multiply cannot fuse into it.
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_coarse_rem(CoarseParams<T> p) {
  __shared__ T a[64], cr[128], ci[128], xs[64];
  const int k = threadIdx.x;
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
  if (s1 < s0 || s1 - s0 != front + (unsigned)__popcll(msk) || s1 > p.ac_count) {      // (wave-uniform) refused, nothing of AC_exact read
    if (k == 0) atomicExch(&p.ctl->error, 2u);
    return;
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
  if (k < l) {
    T val = short_inv_sum(cr, ci, p.rtab, l, k);
    if (p.sf != T(1)) val = val * p.sf;
    xs[k] = val;
  }
  __syncthreads();
  const int f = (int)p.factor;
  const int ncell = (l + f - 1) / f;
  if (k < ncell) {
    const int lo = k * f, hi = min(lo + f, l);
    T acc = xs[lo];
    for (int j = lo + 1; j < hi; j++) acc = acc + xs[j];
    p.out[(size_t)p.nfull * (size_t)(64 / f) + (size_t)k] = acc / (T)(hi - lo);
  }
}

// The instantiation of (mode, geometry, K); coarse_k_ok(geom, k) holds
template <typename T>
auto coarse_kernel(int mode, int geom, int k) -> void (*)(CoarseParams<T>) {
  using Fn = void (*)(CoarseParams<T>);
  return with_mode(mode, [&](auto M) -> Fn {
    if (geom == GEOM_2D) return k == 2 ? k_decompress_coarse_nd<T, M(), GEOM_2D, 2> : k_decompress_coarse_nd<T, M(), GEOM_2D, 4>;
    if (geom == GEOM_3D) return k_decompress_coarse_nd<T, M(), GEOM_3D, 2>;
    switch (k) {
      case 2: return k_decompress_coarse<T, M(), 2>;
      case 4: return k_decompress_coarse<T, M(), 4>;
      case 8: return k_decompress_coarse<T, M(), 8>;
      case 16: return k_decompress_coarse<T, M(), 16>;
      default: return k_decompress_coarse<T, M(), 32>;
    }
  });
}
template <typename T>
int coarse_occupancy(int mode, int geom, int k) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)coarse_kernel<T>(mode, geom, k), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_decompress_coarse(const CoarseParams<T>& p, int mode, int geom, int k, int grid, hipStream_t s) {
  hipLaunchKernelGGL(coarse_kernel<T>(mode, geom, k), dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
void launch_decompress_coarse_rem(const CoarseParams<T>& p, int mode, hipStream_t s) {
  with_mode(mode, [&](auto M) { hipLaunchKernelGGL((k_decompress_coarse_rem<T, M()>), dim3(1), dim3(64), 0, s, p); return 0; });
}
template <typename T>
void launch_decompress_coarse_dc(const float* dc, T* out, unsigned nblk, T sf, hipStream_t s) {
  const unsigned grid = min((nblk + (unsigned)SWG - 1u) / (unsigned)SWG, 4096u);
  hipLaunchKernelGGL(k_decompress_coarse_dc<T>, dim3(grid), dim3(SWG), 0, s, dc, out, nblk, sf);
}
template int coarse_occupancy<double>(int, int, int);
template int coarse_occupancy<float>(int, int, int);
template void launch_decompress_coarse<double>(const CoarseParams<double>&, int, int, int, int, hipStream_t);
template void launch_decompress_coarse<float>(const CoarseParams<float>&, int, int, int, int, hipStream_t);
template void launch_decompress_coarse_rem<double>(const CoarseParams<double>&, int, hipStream_t);
template void launch_decompress_coarse_rem<float>(const CoarseParams<float>&, int, hipStream_t);
template void launch_decompress_coarse_dc<double>(const float*, double*, unsigned, double, hipStream_t);
template void launch_decompress_coarse_dc<float>(const float*, float*, unsigned, float, hipStream_t);

}  // namespace dctz
