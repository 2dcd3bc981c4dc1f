// dctz_kernels_ndcbox.hip -- a box of the coarse decode of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h:
// dctzhip_decompress_coarse_box_nd).
//
// The two parent kernels at once.  From k_decompress_ndbox: with K = edge / factor a block owns the K^d coarse cells
// [b K, b K + K) per axis, so the blocks that hold cells of the box [lo, hi) -- lo / K ... (hi - 1) / K per axis -- are a
// box of the row-major block grid, and BoxGeo::rank over that grid says from launch constants alone whether a stream tile
// (64 consecutive blocks) holds one of them; a tile that holds none is skipped BEFORE anything of it is loaded.  From
// k_decompress_coarse_nd: a hit tile runs coarse_tile_head (all 64 lanes: the flags of blocks outside the box still move
// the places of those behind them), coarse_dequantise, the low-band inverse transform and the de-scale multiply -- the
// whole-array kernel's calls in its order, unfused like everything else: its values, bit for bit -- parks the K^d values
// per block in the LDS image (stride K^d + 1) and walks the row strips with the same step / lane -> (block, offset)
// mapping.  The store is k_decompress_ndbox's: predicated on the box-relative coordinates r = coord - lo, compared
// unsigned against the extent (in front of lo wraps beyond it), 64-bit addressing.  The box lies inside the coarse
// extents, so a cell that begins past the array is never inside it: the whole-array kernel's edge rule needs no test of
// its own here.
//
// k_ndcoarse_mbox (dctz_kernels_mcboxnd.hip: a list of such boxes in one call) carries a COPY of the tile body, from the
// coarse_tile_head call to the closing barrier.  A change to either belongs in both.
//
// k_ndcoarse_box_dc: factor = block edge.  The block grid IS the output grid; the box is gathered from the DC stream alone,
// a thread per output element, consecutive lanes consecutive x, with k_decompress_coarse_dc's expressions in its order.
#include "dctz_coarse_block.h"
#include "dct_lowband_block.h"

namespace dctz {

template <typename T, int MODE, int GEOM, int K>
__global__ __launch_bounds__(64) void k_ndcoarse_box(CoarseBoxParams<T> p) {
  constexpr int KD = CoarseKept<GEOM, K>::N;                            // values per block
  constexpr int ROWS = KD / K;                                         // in-block rows of K values
  constexpr int STRIDE = KD + 1;                                       // odd: the lanes' writes spread over the banks
  __shared__ T img[TILE_BLKS * STRIDE];
  const int lane = threadIdx.x;
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.c.qtab, lane);
  const bool scale = (p.c.sf != T(1));
  const BoxGeo& g = p.blocks;
  const unsigned nbx = p.c.nb[2], nby = p.c.nb[1];
  const unsigned lox = p.lo[2], loy = p.lo[1], loz = p.lo[0];
  const unsigned ex = p.ext[2], ey = p.ext[1], ez = p.ext[0];
  bool bad = false;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1; t += gridDim.x) {
    // hit test over the block grid, from launch constants alone (wave-uniform)
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.c.nfull);
    if (g.rank(b0) == g.rank(b1)) continue;                            // no block of the tile holds a cell of the box: nothing is read
    unsigned w[16];
    float dcv;
    unsigned first, s0;
    if (!coarse_tile_head<T>(p.c, t, lane, w, dcv, first, s0)) { bad = true; continue; }
    T c[KD];
    coarse_dequantise<T, MODE, GEOM, K>(c, w, dcv, p.c.ac + s0, first, qtl, p.c);
    if constexpr (GEOM == GEOM_2D) lowband_inv_2d<T, K>(c); else lowband_inv_3d<T, K>(c);
    if (scale) {
#pragma unroll
      for (int i = 0; i < KD; i++) c[i] = c[i] * p.c.sf;
    }
#pragma unroll
    for (int i = 0; i < KD; i++) img[lane * STRIDE + i] = c[i];
    __syncthreads();
#pragma unroll
    for (unsigned s = 0; s < (unsigned)K; s++) {                       // 64 K strip elements, 64 a step
      const unsigned bl = (unsigned)lane / (unsigned)K + (64u / (unsigned)K) * s;   // block of the tile, offset in its row
      const unsigned off = (unsigned)lane % (unsigned)K;
      const unsigned B = b0 + bl;
      const unsigned q = B / nbx, bx = B - q * nbx;                    // the block's grid coordinates, once per lane and step
      const unsigned bz = GEOM == GEOM_3D ? q / nby : 0u, by = q - bz * nby;
      const unsigned rx = bx * (unsigned)K + off - lox;                // box-relative; unsigned: in front of lo wraps beyond ext
      const bool in = B < b1 && rx < ex;
      const T* const src = img + bl * (unsigned)STRIDE + off;
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const T v = src[r * K];
        const unsigned oz = GEOM == GEOM_3D ? bz * (unsigned)K + (unsigned)(r / K) : 0u;
        const unsigned oy = GEOM == GEOM_3D ? by * (unsigned)K + (unsigned)(r % K) : by * (unsigned)K + (unsigned)r;
        const unsigned rz = oz - loz, ry = oy - loy;
        if (in && rz < ez && ry < ey) p.c.out[((size_t)rz * ey + ry) * ex + rx] = v;
      }
    }
    __syncthreads();                                                   // the image is read out before the next tile writes it
  }
  if (bad && lane == 0) atomicExch(&p.c.ctl->error, 2u);
}

// factor = block edge: K = 1, the box [lo, lo + ext) of the block grid nb from the DC stream (k_decompress_coarse_dc's expressions)
template <typename T>
__global__ __launch_bounds__(SWG) void k_ndcoarse_box_dc(const float* __restrict__ dc, T* __restrict__ out, const unsigned nby, const unsigned nbx,
                                                         const unsigned loz, const unsigned loy, const unsigned lox, const unsigned ey,
                                                         const unsigned ex, const unsigned cnt, const T sf) {
  const bool scale = (sf != T(1));
  for (unsigned o = blockIdx.x * (unsigned)SWG + threadIdx.x; o < cnt; o += gridDim.x * (unsigned)SWG) {
    const unsigned q = o / ex, rx = o - q * ex;
    const unsigned rz = q / ey, ry = q - rz * ey;
    const size_t b = ((size_t)(loz + rz) * nby + (loy + ry)) * nbx + (lox + rx);
    T v = (T)dc[b] * T(0.125);
    if (scale) v = v * sf;
    out[o] = v;
  }
}

// The instantiation of (mode, geometry, K); ndcbox_k_ok(geom, k) holds
template <typename T>
auto ndcbox_kernel(int mode, int geom, int k) -> void (*)(CoarseBoxParams<T>) {
  using Fn = void (*)(CoarseBoxParams<T>);
  return with_mode(mode, [&](auto M) -> Fn {
    if (geom == GEOM_3D) return k_ndcoarse_box<T, M(), GEOM_3D, 2>;
    return k == 2 ? k_ndcoarse_box<T, M(), GEOM_2D, 2> : k_ndcoarse_box<T, M(), GEOM_2D, 4>;
  });
}
template <typename T>
int ndcbox_occupancy(int mode, int geom, int k) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)ndcbox_kernel<T>(mode, geom, k), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_ndcoarse_box(const CoarseBoxParams<T>& p, int mode, int geom, int k, int grid, hipStream_t s) {
  hipLaunchKernelGGL(ndcbox_kernel<T>(mode, geom, k), dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
unsigned launch_ndcoarse_box_dc(const float* dc, T* out, const unsigned (&nb)[3], const unsigned (&lo)[3], const unsigned (&ext)[3], T sf,
                                hipStream_t s) {
  const unsigned cnt = ext[0] * ext[1] * ext[2];
  const unsigned grid = min((cnt + (unsigned)SWG - 1u) / (unsigned)SWG, 4096u);
  hipLaunchKernelGGL(k_ndcoarse_box_dc<T>, dim3(grid), dim3(SWG), 0, s, dc, out, nb[1], nb[2], lo[0], lo[1], lo[2], ext[1], ext[2], cnt, sf);
  return grid;
}
template int ndcbox_occupancy<double>(int, int, int);
template int ndcbox_occupancy<float>(int, int, int);
template void launch_ndcoarse_box<double>(const CoarseBoxParams<double>&, int, int, int, int, hipStream_t);
template void launch_ndcoarse_box<float>(const CoarseBoxParams<float>&, int, int, int, int, hipStream_t);
template unsigned launch_ndcoarse_box_dc<double>(const float*, double*, const unsigned (&)[3], const unsigned (&)[3], const unsigned (&)[3], double, hipStream_t);
template unsigned launch_ndcoarse_box_dc<float>(const float*, float*, const unsigned (&)[3], const unsigned (&)[3], const unsigned (&)[3], float, hipStream_t);

}  // namespace dctz
