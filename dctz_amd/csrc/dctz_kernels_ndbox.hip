// dctz_kernels_ndbox.hip -- a box of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h:
// dctzhip_decompress_box_nd).
//
// A block of these streams IS a small box of the array (an 8 x 8 or 4 x 4 x 4 brick), the blocks are numbered row-major
// over the block grid, and 64 consecutive blocks make a stream tile: 4096 positions, one entry of the exception index.
// The blocks that intersect the box form a box of the block grid, so the hit test of k_decompress_box carries over with
// the block grid in place of the array: BoxGeo::rank counts the intersecting blocks in front of block 64 t and in front
// of the tile's end; equal: the tile is skipped BEFORE anything is loaded.  A hit tile is decoded once by ra_tile_image
// with the geometry's separable inverse transform (the text every decoder of dctzhip_decompress_nd runs: bit for bit its
// elements) and leaves through the LDS image.
//
// Scatter.  Lane b's 64 values are a brick, not a run of d_out; but the blocks of a tile neighbour along the fastest
// axis, so in-block row r of all 64 blocks is a ROW STRIP of 64 e consecutive array elements (e = 8 | 4, up to where the
// tile wraps into the next block row).  The strip is read back from the image 64 elements at a time: step s, lane l ->
// strip element i = l + 64 s = block i / e, in-row offset i % e.  The block's grid coordinates come from one
// decomposition per lane and step, outside the loop over the in-block rows; a store is predicated on "inside the box" and
// addressed by box-relative coordinates with 64-bit pointer arithmetic (an fp64 box may exceed 4 GiB).  The stores of one
// instruction are consecutive across the lanes: e lanes per block, 64 / e neighbouring blocks.  Padded positions of edge
// blocks have a coordinate >= dims >= hi and are never stored.
// (The baseline -- lane b stores its own block's rows, e consecutive elements per lane, 64 lines per instruction --
// measured slower on the brick and the x-plane: EXPERIMENTS section 22.)
//
// The image's row stride (NdImage, dctz_nd_image.h) is chosen for this walk from the LDS banking table of gfx950 (DESIGN
// section 13).
#include "dctz_nd_image.h"

namespace dctz {

template <typename T, int MODE, int GEOM>
__global__ __launch_bounds__(64) void k_decompress_ndbox(NdBoxParams<T> p) {
  using G = NdImage<T, GEOM>;
  constexpr unsigned E = GEOM == GEOM_2D ? 8u : 4u;                    // block edge
  constexpr int ROWS = 64 / (int)E;                                    // in-block rows of E elements
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::BYTES];
  const T* const img = reinterpret_cast<const T*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const BoxGeo& g = p.blocks;
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned lox = p.lo[2], loy = p.lo[1], loz = p.lo[0];
  const unsigned ex = p.ext[2], ey = p.ext[1], ez = p.ext[0];
  bool bad = false;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    // hit test over the block grid, from launch constants alone (wave-uniform)
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.nfull);
    if (g.rank(b0) == g.rank(b1)) continue;                            // no block of the tile meets the box: nothing is read
    if (!ra_tile_image<T, MODE, GEOM, G>(p, t, lane, tab, qtl, scale, lds)) { bad = true; continue; }
#pragma unroll
    for (unsigned s = 0; s < E; s++) {                                 // 64 E strip elements, 64 a step
      const unsigned bl = (unsigned)lane / E + (64u / E) * s;          // block of the tile, in-row offset
      const unsigned off = (unsigned)lane % E;
      const unsigned B = b0 + bl;
      const unsigned q = B / nbx, bx = B - q * nbx;                    // the block's grid coordinates, once per lane and step
      const unsigned bz = GEOM == GEOM_3D ? q / nby : 0u, by = q - bz * nby;
      const unsigned rx = bx * E + off - lox;                          // box-relative; unsigned: in front of lo wraps beyond ext
      const bool in = B < b1 && rx < ex;
      const T* const src = img + bl * (unsigned)G::STRIDE + off;
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        const T v = src[r * (int)E];
        const unsigned z = GEOM == GEOM_3D ? bz * 4u + (unsigned)(r >> 2) : 0u;
        const unsigned y = GEOM == GEOM_3D ? by * 4u + (unsigned)(r & 3) : by * 8u + (unsigned)r;
        const unsigned rz = z - loz, ry = y - loy;
        if (in && rz < ez && ry < ey) p.out[((size_t)rz * ey + ry) * ex + rx] = v;
      }
    }
    __syncthreads();                                                   // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

template <typename T>
auto ndbox_kernel(int mode, int geom) -> void (*)(NdBoxParams<T>) {
  return with_mode_bool(mode, geom == GEOM_3D, [](auto M, auto D3) { return k_decompress_ndbox<T, M(), D3() ? GEOM_3D : GEOM_2D>; });
}
template <typename T>
int ndbox_occupancy(int mode, int geom) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)ndbox_kernel<T>(mode, geom), 64, 0);
  return e == hipSuccess ? n : 0;
}

template <typename T>
void launch_decompress_ndbox(const NdBoxParams<T>& p, int mode, int geom, int grid, hipStream_t s) {
  hipLaunchKernelGGL(ndbox_kernel<T>(mode, geom), dim3(grid), dim3(64), 0, s, p);
}
template int ndbox_occupancy<double>(int, int);
template int ndbox_occupancy<float>(int, int);
template void launch_decompress_ndbox<double>(const NdBoxParams<double>&, int, int, int, hipStream_t);
template void launch_decompress_ndbox<float>(const NdBoxParams<float>&, int, int, int, hipStream_t);

}  // namespace dctz
