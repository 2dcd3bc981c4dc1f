// dctz_kernels_mboxnd.hip -- a list of boxes of one array compressed in 8 x 8 / 4 x 4 x 4 tiles, in one call
// (include/dctz_hip.h: dctzhip_decompress_boxes_nd).
//
// dctzhip_decompress_box_nd gives every CANDIDATE stream tile of its box a workgroup; of the 64^3 brick of a 512^3 volume
// 512 of 3872 candidates are hit.  Here the hit test runs first, for all boxes at once, by the flat list call's own
// builder: k_boxlist_build (dctz_kernels_mbox.hip, unchanged) is handed the box of the BLOCK grid of every box (BoxRec::g
// = NdBoxParams::blocks), unit = TILE_BLKS blocks and end = nblk, and compacts the hit (box, stream tile) pairs into the
// list.  k_decompress_mbox_nd's single-wave workgroups then take items w, w + G, ... up to the count the builder left in
// the control block: every workgroup decodes hit tiles only.  Per item the output pointer of the box's record and the box
// in elements (NdBoxElems) are read by wave-uniform loads into scalar registers; the blocks per axis stay launch constants.
//
// The tile body is k_decompress_ndbox's (dctz_kernels_ndbox.hip) from its ra_tile_image call to its closing barrier, with
// the record's box and output in place of the launch constants.  It is a COPY, as k_decompress_mbox's is of
// k_decompress_box: that kernel's text stays as it was measured (EXPERIMENTS.md, "Many boxes of a tiled array").  A change
// to either belongs in both.  There is no short block (n = 64 nblk), so no _rem kernel.
#include "dctz_nd_image.h"
#include "dctz_uniform_words.h"

namespace dctz {
// (a namespace of its own: the kernel's qualified name is dctz::tiled::k_decompress_mbox_nd, so that a listing of the flat
// call's kernels by the prefix dctz::k_decompress_mbox keeps showing those alone)
namespace tiled {

template <typename T, int MODE, int GEOM>
__global__ __launch_bounds__(64) void k_decompress_mbox_nd(MBoxNdParams<T> p) {
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
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned count = min((unsigned)__builtin_amdgcn_readfirstlane((int)p.ctl->cnt_total), p.cap);
  bool bad = false;
  for (unsigned i = blockIdx.x; i < count; i += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].box);
    const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].tile);
    T* const out = static_cast<T*>(uniform_words(&p.recs[b].out));
    const NdBoxElems e = uniform_words(p.elems + b);
    const unsigned lox = e.lo[2], loy = e.lo[1], loz = e.lo[0];
    const unsigned ex = e.ext[2], ey = e.ext[1], ez = e.ext[0];
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.nfull);
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
        if (in && rz < ez && ry < ey) out[((size_t)rz * ey + ry) * ex + rx] = v;
      }
    }
    __syncthreads();                                                   // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

}  // namespace tiled

template <typename T>
auto mboxnd_kernel(int mode, int geom) -> void (*)(MBoxNdParams<T>) {
  return with_mode_bool(mode, geom == GEOM_3D, [](auto M, auto D3) { return tiled::k_decompress_mbox_nd<T, M(), D3() ? GEOM_3D : GEOM_2D>; });
}
template <typename T>
int mboxnd_occupancy(int mode, int geom) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mboxnd_kernel<T>(mode, geom), 64, 0);
  return e == hipSuccess ? n : 0;
}

template <typename T>
void launch_decompress_mbox_nd(const MBoxNdParams<T>& p, int mode, int geom, int grid, hipStream_t s) {
  hipLaunchKernelGGL(mboxnd_kernel<T>(mode, geom), dim3(grid), dim3(64), 0, s, p);
}
template int mboxnd_occupancy<double>(int, int);
template int mboxnd_occupancy<float>(int, int);
template void launch_decompress_mbox_nd<double>(const MBoxNdParams<double>&, int, int, int, hipStream_t);
template void launch_decompress_mbox_nd<float>(const MBoxNdParams<float>&, int, int, int, hipStream_t);

}  // namespace dctz
