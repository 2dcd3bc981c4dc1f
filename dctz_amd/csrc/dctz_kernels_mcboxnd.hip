// dctz_kernels_mcboxnd.hip -- a list of boxes of the coarse decode of one array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one
// call (include/dctz_hip.h: dctzhip_decompress_coarse_boxes_nd).
//
// dctzhip_decompress_coarse_box_nd gives every CANDIDATE stream tile of its box a workgroup and pays a launch and a read-back
// per box.  Here the hit test runs first, for all boxes at once, by the list calls' own builder: k_boxlist_build
// (dctz_kernels_mbox.hip, unchanged) is handed the box of the BLOCK grid of every box (BoxRec::g = CoarseBoxParams::blocks:
// with K = edge / factor a block owns the K^d coarse cells [b K, b K + K) per axis), unit = TILE_BLKS blocks and end = nblk,
// and compacts the hit (box, stream tile) pairs into the list.  k_ndcoarse_mbox's single-wave workgroups then take items w,
// w + G, ... up to the count the builder left in the control block: every workgroup decodes hit tiles only.  Per item the
// output pointer of the box's record and the box in coarse cells (NdBoxElems) are read by wave-uniform loads into scalar
// registers; the blocks per axis stay launch constants.
//
// The tile body is k_ndcoarse_box's (dctz_kernels_ndcbox.hip) from its coarse_tile_head call to its closing barrier, with the
// record's box and output in place of the launch constants: the whole-array kernel's calls in its order, unfused, so its
// values bit for bit.  It is a COPY, as k_decompress_mbox_nd's is of k_decompress_ndbox: that kernel's text stays as it was
// measured.  A change to either belongs in both.
//
// k_ndcoarse_mbox_dc: factor = block edge.  The block grid IS the output grid; ONE launch gathers all k boxes from the DC
// stream alone -- blockIdx.y is the box, a grid-stride loop in x over its cells -- with k_ndcoarse_box_dc's expressions in
// its order.  No list, no builder.
#include "dctz_coarse_block.h"
#include "dct_lowband_block.h"
#include "dctz_uniform_words.h"

namespace dctz {
// (a namespace of its own: the kernels' qualified names are dctz::tiled::k_ndcoarse_mbox..., so that a listing of the single
// call's kernels by the prefix dctz::k_ndcoarse_box keeps showing those alone)
namespace tiled {

template <typename T, int MODE, int GEOM, int K>
__global__ __launch_bounds__(64) void k_ndcoarse_mbox(MCBoxNdParams<T> p) {
  constexpr int KD = CoarseKept<GEOM, K>::N;                            // values per block
  constexpr int ROWS = KD / K;                                         // in-block rows of K values
  constexpr int STRIDE = KD + 1;                                       // odd: the lanes' writes spread over the banks
  __shared__ T img[TILE_BLKS * STRIDE];
  const int lane = threadIdx.x;
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.c.qtab, lane);
  const bool scale = (p.c.sf != T(1));
  const unsigned nbx = p.c.nb[2], nby = p.c.nb[1];
  const unsigned count = min((unsigned)__builtin_amdgcn_readfirstlane((int)p.c.ctl->cnt_total), p.cap);
  bool bad = false;
  for (unsigned i = blockIdx.x; i < count; i += gridDim.x) {
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].box);
    const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].tile);
    T* const out = static_cast<T*>(uniform_words(&p.recs[b].out));
    const NdBoxElems e = uniform_words(p.elems + b);
    const unsigned lox = e.lo[2], loy = e.lo[1], loz = e.lo[0];
    const unsigned ex = e.ext[2], ey = e.ext[1], ez = e.ext[0];
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.c.nfull);
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
        if (in && rz < ez && ry < ey) out[((size_t)rz * ey + ry) * ex + rx] = v;
      }
    }
    __syncthreads();                                                   // the image is read out before the next item writes it
  }
  if (bad && lane == 0) atomicExch(&p.c.ctl->error, 2u);
}

// factor = block edge: K = 1, box blockIdx.y [lo, lo + ext) of the block grid from the DC stream (k_ndcoarse_box_dc's
// expressions).  A box holds at most nblk < 2^25 cells: its count stays an unsigned.
template <typename T>
__global__ __launch_bounds__(SWG) void k_ndcoarse_mbox_dc(const float* __restrict__ dc, const BoxRec* __restrict__ recs,
                                                          const NdBoxElems* __restrict__ elems, const unsigned nby, const unsigned nbx,
                                                          const T sf) {
  const bool scale = (sf != T(1));
  T* const out = static_cast<T*>(uniform_words(&recs[blockIdx.y].out));
  const NdBoxElems e = uniform_words(elems + blockIdx.y);
  const unsigned ex = e.ext[2], ey = e.ext[1];
  const unsigned cnt = e.ext[0] * ey * ex;
  for (unsigned o = blockIdx.x * (unsigned)SWG + threadIdx.x; o < cnt; o += gridDim.x * (unsigned)SWG) {
    const unsigned q = o / ex, rx = o - q * ex;
    const unsigned rz = q / ey, ry = q - rz * ey;
    const size_t b = ((size_t)(e.lo[0] + rz) * nby + (e.lo[1] + ry)) * nbx + (e.lo[2] + rx);
    T v = (T)dc[b] * T(0.125);
    if (scale) v = v * sf;
    out[o] = v;
  }
}

}  // namespace tiled

// The instantiation of (mode, geometry, K), for the launch and the occupancy query alike; ndcbox_k_ok(geom, k) holds
template <typename T>
auto mcboxnd_kernel(int mode, int geom, int k) -> void (*)(MCBoxNdParams<T>) {
  using Fn = void (*)(MCBoxNdParams<T>);
  return with_mode(mode, [&](auto M) -> Fn {
    if (geom == GEOM_3D) return tiled::k_ndcoarse_mbox<T, M(), GEOM_3D, 2>;
    return k == 2 ? tiled::k_ndcoarse_mbox<T, M(), GEOM_2D, 2> : tiled::k_ndcoarse_mbox<T, M(), GEOM_2D, 4>;
  });
}
template <typename T>
int mcboxnd_occupancy(int mode, int geom, int k) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mcboxnd_kernel<T>(mode, geom, k), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_ndcoarse_mbox(const MCBoxNdParams<T>& p, int mode, int geom, int k, int grid, hipStream_t s) {
  hipLaunchKernelGGL(mcboxnd_kernel<T>(mode, geom, k), dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
unsigned launch_ndcoarse_mbox_dc(const float* dc, const BoxRec* recs, const NdBoxElems* elems, unsigned nbox, unsigned max_cells,
                                 const unsigned (&nb)[3], T sf, hipStream_t s) {
  // about 4096 workgroups in all, and no more per box than its largest needs
  const unsigned gx = std::max(1u, std::min((max_cells + (unsigned)SWG - 1u) / (unsigned)SWG, 4096u / nbox));
  hipLaunchKernelGGL(tiled::k_ndcoarse_mbox_dc<T>, dim3(gx, nbox), dim3(SWG), 0, s, dc, recs, elems, nb[1], nb[2], sf);
  return gx * nbox;
}
template int mcboxnd_occupancy<double>(int, int, int);
template int mcboxnd_occupancy<float>(int, int, int);
template void launch_ndcoarse_mbox<double>(const MCBoxNdParams<double>&, int, int, int, int, hipStream_t);
template void launch_ndcoarse_mbox<float>(const MCBoxNdParams<float>&, int, int, int, int, hipStream_t);
template unsigned launch_ndcoarse_mbox_dc<double>(const float*, const BoxRec*, const NdBoxElems*, unsigned, unsigned, const unsigned (&)[3], double, hipStream_t);
template unsigned launch_ndcoarse_mbox_dc<float>(const float*, const BoxRec*, const NdBoxElems*, unsigned, unsigned, const unsigned (&)[3], float, hipStream_t);

}  // namespace dctz
