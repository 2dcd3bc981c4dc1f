// dctz_kernels_box.hip -- a rectangular sub-region of an N-D array in one call (include/dctz_hip.h: dctzhip_decompress_box).
//
// The array is compressed in flat 64-element blocks, 64 blocks to a tile; a box of it is many short runs of the flat order,
// but they lie in few tiles.  k_decompress_box takes the candidate tiles [t0, t1) (those of the first and the last box
// element), one single-wave workgroup each, and asks of every tile, BEFORE it loads anything: how many box elements lie in
// front of its first element, how many in front of its end (BoxGeo::rank, dctz_device.h).  Equal: the tile is not hit and
// is skipped whole.  Otherwise the tile is decoded once by ra_tile_image (dctz_kernel_common.h: the text k_decompress_range
// runs, so every element is bit for bit dctzhip_decompress's), and -- since the flat order restricted to the box is the
// box's own C order -- its box elements are the CONSECUTIVE output positions [oa, ob) between the two counts.  The lanes
// walk those positions: box coordinates by one decomposition per lane and tile, then 64 further per step with one carry per
// dimension, the flat position by additions alone (BoxGeo::fstep, wrap); the element is read from the tile's LDS image and
// stored through a buffer descriptor that covers exactly d_out[oa, ob).  Work per tile follows its elements in the box,
// stores are consecutive across the lanes.
// The short last block is k_decompress_box_rem's (dctz_kernel_common.h: box_rem_block, shared with the list call), as
// k_decompress_range_rem with the box test in place of [lo, hi).
#include "dctz_kernel_common.h"

namespace dctz {

template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_box(BoxParams<T> p) {
  using G = RaGeo<T>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::BYTES];
  const T* const img = reinterpret_cast<const T*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const unsigned full_end = p.nfull * 64u;
  const BoxGeo& g = p.box;
  bool bad = false;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    // hit test, from launch constants alone (wave-uniform)
    const unsigned ts = t * (unsigned)TILE_ELEMS;
    const unsigned te = min(ts + (unsigned)TILE_ELEMS, p.n);
    const unsigned oa = g.rank(ts);
    const unsigned oe = g.rank(te);
    if (oe == oa) continue;                                            // no element of the tile lies in the box: nothing is read
    if (!ra_tile_image<T, MODE>(p, t, lane, tab, qtl, scale, lds)) { bad = true; continue; }
    // the tile's whole-block elements inside the box -> d_out[oa, ob)
    const unsigned ob = te > full_end ? g.rank(max(full_end, ts)) : oe;
    if (oa < ob) {
      // (a descriptor per tile: d_out[oa, ob) and not a byte more -- num_records is 32 bits, a box may be larger)
      const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out + oa, 0, (int)((ob - oa) * sizeof(T)), 0x00020000);
      unsigned o = oa + (unsigned)lane;
      if (o < ob) {
        unsigned b[BOX_ND];
        unsigned f = g.flat_of(o, b);
        for (;;) {
          const T v = img[G::at(f - ts)];
          const int at = (int)((o - oa) * (unsigned)sizeof(T));
          if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r_out, at, 0, 0);
          else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r_out, at, 0, 0);
          o += 64u;
          if (o >= ob) break;
          unsigned carry = 0, df = g.fstep;
#pragma unroll
          for (int d = BOX_ND - 1; d > 0; d--) {                       // b + step < 2 ext: one carry per dimension
            b[d] += g.step[d] + carry;
            carry = b[d] >= g.ext[d] ? 1u : 0u;
            b[d] -= carry ? g.ext[d] : 0u;
            df += carry ? g.wrap[d] : 0u;
          }
          f += df;
        }
      }
    }
    __syncthreads();                                                   // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The short last block (length l = n % 64) when the box reaches into it: k_decompress_range_rem with the box test and the
// box's output position in place of [lo, hi).
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_box_rem(BoxParams<T> p) {
  __shared__ T a[64];
  __shared__ T cr[128];
  __shared__ T ci[128];
  box_rem_block<T, MODE>(p, p.box, p.out, (int)threadIdx.x, a, cr, ci);
}

template <typename T>
auto box_kernel(int mode) -> void (*)(BoxParams<T>) {
  return with_mode(mode, [](auto M) { return k_decompress_box<T, M()>; });
}
template <typename T>
int box_occupancy(int mode) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)box_kernel<T>(mode), 64, 0);
  return e == hipSuccess ? n : 0;
}

template <typename T>
void launch_decompress_box(const BoxParams<T>& p, int mode, int grid, bool with_rem, hipStream_t s) {
  if (grid > 0) hipLaunchKernelGGL(box_kernel<T>(mode), dim3(grid), dim3(64), 0, s, p);
  if (with_rem) hipLaunchKernelGGL(with_mode(mode, [](auto M) { return k_decompress_box_rem<T, M()>; }), dim3(1), dim3(64), 0, s, p);
}
template int box_occupancy<double>(int);
template int box_occupancy<float>(int);
template void launch_decompress_box<double>(const BoxParams<double>&, int, int, bool, hipStream_t);
template void launch_decompress_box<float>(const BoxParams<float>&, int, int, bool, hipStream_t);

}  // namespace dctz
