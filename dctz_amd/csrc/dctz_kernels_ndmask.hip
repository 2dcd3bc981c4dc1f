// dctz_kernels_ndmask.hip -- the missing-value layer for arrays compressed in 8 x 8 / 4 x 4 x 4 tiles: the mask of the array
// in C element order and the holes filled by copies inside each tile (include/dctz_hip.h: dctzhip_mask_build_nd; DESIGN
// section 13).
//
// k_ndmask_fill: k_mask_fill with other addresses.  A lane takes 16 bytes (E = 2 fp64 or 4 fp32 elements) of one tile row,
// and the L = 64 / E lanes of a tile stand in ascending in-tile place j, so lane order is block order and the fill inside a
// block is the flat kernel's (dctz_mask_fill.h).  A wave trip is E tiles that are neighbours along the fastest axis: in 2-D
// every row of a trip is one 128-byte line, in 3-D half a line, and the MASK_TRIPS trips whose loads a wave issues before it
// looks at the first follow each other along that axis, so the same wave completes the lines.  A trip inside the array whose
// row pitch keeps 16-byte alignment moves as 16-byte pieces; every other trip (edge tiles, odd pitches) element by element
// under the lane's presence bits, and a padded position is neither read nor written nor a source.  The mask: the bits of a
// trip row are joined across its lanes by an OR butterfly; where every trip row is whole aligned bytes of the mask (p.plain)
// its first lane stores them, else the mask was cleared in stream order and the rows are ORed in with vector atomics -- the
// bytes are the same on every grid either way.  The count is an integer sum (a wave reduction and one atomic per wave).
#include "dctz_mask_fill.h"

namespace dctz {

template <int BITS> struct MaskPiece { using P = unsigned; };
template <> struct MaskPiece<16> { using P = unsigned short; };
template <> struct MaskPiece<8> { using P = unsigned char; };

template <typename T, int GEOM>
__global__ __launch_bounds__(MASK_WG) void k_ndmask_fill(NdMaskFillParams<T> p) {
  using U = typename MaskBits<T>::U;
  constexpr int E = 16 / (int)sizeof(T);             // elements of a lane
  constexpr int L = 64 / E;                          // lanes of a tile
  constexpr int EDGE = GEOM == GEOM_2D ? 8 : 4;
  constexpr int R = EDGE / E;                        // lanes of a tile row
  constexpr unsigned W = (unsigned)(EDGE * E);       // elements of a trip row = bits of its piece of the mask: 8, 16 or 32
  constexpr unsigned FULL = (1u << E) - 1u;
  using P = typename MaskPiece<(int)W>::P;
  const int lane = threadIdx.x & 63;
  const unsigned wave = blockIdx.x * (unsigned)(MASK_WG / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (unsigned)(MASK_WG / 64);
  // the lane's place: tile t of the trip, row rr of the tile (j = EDGE rr + E h ...), piece h of the row
  const unsigned t = (unsigned)lane / L, q = (unsigned)lane % L, rr = q / R, h = q % R;
  const unsigned lx = t * EDGE + h * E, ly = GEOM == GEOM_2D ? rr : rr & 3u, lz = GEOM == GEOM_2D ? 0u : rr >> 2;
  const bool holder = lane < L && h == 0u;           // the first lane of a trip row: it writes the row's bits
  // (the filled copy may BE the input: no __restrict__; a lane reads its elements before it writes them, and only those)
  const U* const in = reinterpret_cast<const U*>(p.in);
  U* const out = reinterpret_cast<U*>(p.out);
  const unsigned groups = (p.trips + MASK_TRIPS - 1u) / MASK_TRIPS;
  unsigned cnt = 0;
  for (unsigned g = wave; g < groups; g += nwaves) {
    U x[MASK_TRIPS][E];
    unsigned e0[MASK_TRIPS], present[MASK_TRIPS];
    const unsigned tr = g * MASK_TRIPS;
    unsigned tx = tr % p.ntx, by = tr / p.ntx % p.nby, bz = tr / p.ntx / p.nby;
    // MASK_TRIPS trips' loads in flight per lane before the first of them is looked at
#pragma unroll
    for (int u = 0; u < MASK_TRIPS; u++) {
      const bool there = tr + u < p.trips;           // (all of this but the lane's own coordinates is wave-uniform)
      const unsigned z = GEOM == GEOM_2D ? 0u : bz * 4u + lz, y = by * EDGE + ly, xx = tx * W + lx;
      e0[u] = (z * p.dy + y) * p.dx + xx;            // (beyond the array: never used)
      const bool whole = there && p.pitch16 && tx * W + W <= p.dx && by * EDGE + EDGE <= p.dy && (GEOM == GEOM_2D || bz * 4u + 4u <= p.dz);
      if (whole) {
        present[u] = FULL;
        const u32x4 v = *reinterpret_cast<const u32x4*>(in + e0[u]);
        __builtin_memcpy(x[u], &v, 16);
      } else {
        const bool real = there && z < p.dz && y < p.dy && xx < p.dx;
        present[u] = !real ? 0u : xx + E <= p.dx ? FULL : (1u << (p.dx - xx)) - 1u;
#pragma unroll
        for (int k = 0; k < E; k++) x[u][k] = (present[u] >> k) & 1u ? in[e0[u] + k] : U(0);
      }
      if (++tx == p.ntx) { tx = 0; if (++by == p.nby) { by = 0; bz++; } }
    }
#pragma unroll
    for (int u = 0; u < MASK_TRIPS; u++) {
      const unsigned miss = mask_settle<T>(x[u], present[u], p.flags, p.value, p.limit);
      cnt += (unsigned)__popc(miss);
      // the mask: this lane's bits at their place in the trip row, joined across the row's lanes in every tile of the trip
      unsigned w = miss << lx;
#pragma unroll
      for (int d = 1; d < R; d <<= 1) w |= (unsigned)__shfl_xor((int)w, d);
#pragma unroll
      for (int d = L; d < 64; d <<= 1) w |= (unsigned)__shfl_xor((int)w, d);
      if (holder && present[u]) {                    // a real row; its bits start at bit e0 < n of the mask
        if (p.plain) {                               // e0 is a multiple of W and the row has all its W elements
          reinterpret_cast<P*>(p.mask32)[e0[u] / W] = (P)w;
        } else if (w) {
          const unsigned long long v = (unsigned long long)w << (e0[u] & 31u);
          if ((unsigned)v) atomicOr(p.mask32 + (e0[u] >> 5), (unsigned)v);
          if ((unsigned)(v >> 32)) atomicOr(p.mask32 + (e0[u] >> 5) + 1u, (unsigned)(v >> 32));   // (a set bit lies below n)
        }
      }
      if (!out) continue;                            // (wave-uniform) mask and count only
      mask_fill_block<T>(x[u], present[u] & ~miss, lane);
      mask_store_lane<T>(out, e0[u], x[u], present[u], p.pitch16 && present[u] == FULL);
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, d);
  if (lane == 0 && cnt) atomicAdd(&p.ctl->cnt_total, cnt);
}

// The instantiation of a geometry
template <typename T>
auto ndmask_kernel(int geom) -> void (*)(NdMaskFillParams<T>) {
  return geom == GEOM_3D ? k_ndmask_fill<T, GEOM_3D> : k_ndmask_fill<T, GEOM_2D>;
}
template <typename T>
void launch_ndmask_fill(const NdMaskFillParams<T>& p, int geom, int grid, hipStream_t s) {
  hipLaunchKernelGGL(ndmask_kernel<T>(geom), dim3(grid), dim3(MASK_WG), 0, s, p);
}
template void launch_ndmask_fill<double>(const NdMaskFillParams<double>&, int, int, hipStream_t);
template void launch_ndmask_fill<float>(const NdMaskFillParams<float>&, int, int, hipStream_t);

}  // namespace dctz
