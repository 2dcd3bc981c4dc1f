// dctz_kernels_mask.hip -- the missing-value layer: a bit per element beside the streams, the holes filled by copies before
// the array is compressed and written back with the caller's fill after any decode (include/dctz_hip.h: dctzhip_mask_build /
// dctzhip_mask_apply).
//
// k_mask_fill: a pure stream.  A lane takes 16 bytes (E = 2 fp64 or 4 fp32 elements), so a codec block is L = 32 or 16
// neighbouring lanes and a wave trip covers E blocks in whole lines, read and written; a wave issues the loads of MASK_TRIPS
// trips before it looks at the first.  The fill rule needs no scan: a lane settles its own E elements in registers and asks
// the ballot of "this lane holds a valid element" for the nearest such lane in front of it in its block (else the first one
// of the block), whose last (first) valid element it fetches.  The mask leaves as 32-bit pieces, the lanes' E bits joined by
// an OR butterfly over the 32 / E lanes of a piece.  The count is an integer sum (a wave reduction and one atomic per wave);
// nothing else depends on the grid.
// k_mask_apply: a lane per element of the dense box; the element's flat position gives its bit; set bits store the fill.
#include "dctz_mask_fill.h"          // the fill inside one block, shared with k_ndmask_fill

namespace dctz {

// One trip of a wave: the 64 E elements from element ch * 64 E on.  x holds this lane's E elements as bit patterns (zeros
// where `present` has no bit: beyond the array's end); the lane's count of missing elements is returned.
template <typename T>
__device__ __forceinline__ unsigned mask_fill_trip(const MaskFillParams<T>& p, const unsigned ch, const int lane, typename MaskBits<T>::U (&x)[16 / sizeof(T)],
                                                   const unsigned present) {
  using U = typename MaskBits<T>::U;
  constexpr int E = 16 / (int)sizeof(T);             // elements of a lane
  constexpr int PL = 32 / E;                         // lanes of a 32-bit piece of the mask
  const unsigned e0 = ch * (64u * E) + (unsigned)lane * E;
  const unsigned miss = mask_settle<T>(x, present, p.flags, p.value, p.limit);
  const unsigned valid = present & ~miss;
  // the mask: this lane's bits at their place in the piece, joined across the piece's lanes
  unsigned w = miss << (E * (lane & (PL - 1)));
#pragma unroll
  for (int d = 1; d < PL; d <<= 1) w |= (unsigned)__shfl_xor((int)w, d);
  const unsigned piece = ch * (2u * E) + (unsigned)(lane / PL);
  if ((lane & (PL - 1)) == 0 && piece < (p.n + 63u) / 64u * 2u) p.mask32[piece] = w;     // two pieces per word of the mask
  U* const out = reinterpret_cast<U*>(p.out);
  if (!out) return (unsigned)__popc(miss);           // (wave-uniform) mask and count only
  mask_fill_block<T>(x, valid, lane);
  mask_store_lane<T>(out, e0, x, present, present == (1u << E) - 1u);
  return (unsigned)__popc(miss);
}

template <typename T>
__global__ __launch_bounds__(MASK_WG) void k_mask_fill(MaskFillParams<T> p) {
  using U = typename MaskBits<T>::U;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr unsigned CHUNK = 64u * E;                // elements of a wave's trip
  const int lane = threadIdx.x & 63;
  const unsigned wave = blockIdx.x * (unsigned)(MASK_WG / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (unsigned)(MASK_WG / 64);
  const unsigned chunks = (p.n + CHUNK - 1u) / CHUNK;
  const unsigned groups = p.n / (CHUNK * MASK_TRIPS);   // of MASK_TRIPS whole trips
  // (the filled copy may BE the input: no __restrict__; a lane reads its 16 bytes before it writes them, and only those)
  const U* const in = reinterpret_cast<const U*>(p.in);
  unsigned cnt = 0;
  // MASK_TRIPS loads in flight per lane before the first of them is looked at: a wave with one is bound by the latency
  for (unsigned g = wave; g < groups; g += nwaves) {
    U x[MASK_TRIPS][E];
#pragma unroll
    for (int u = 0; u < MASK_TRIPS; u++) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((g * MASK_TRIPS + u) * CHUNK + (unsigned)lane * E));
      __builtin_memcpy(x[u], &v, 16);
    }
#pragma unroll
    for (int u = 0; u < MASK_TRIPS; u++) cnt += mask_fill_trip<T>(p, g * MASK_TRIPS + u, lane, x[u], (1u << E) - 1u);
  }
  // what is left: fewer than MASK_TRIPS whole trips and the one the array ends in
  for (unsigned ch = groups * MASK_TRIPS + wave; ch < chunks; ch += nwaves) {
    const unsigned e0 = ch * CHUNK + (unsigned)lane * E;
    const unsigned present = e0 + E <= p.n ? (1u << E) - 1u : e0 < p.n ? (1u << (p.n - e0)) - 1u : 0u;
    U x[E];
#pragma unroll
    for (int k = 0; k < E; k++) x[k] = (present >> k) & 1u ? in[e0 + k] : U(0);
    cnt += mask_fill_trip<T>(p, ch, lane, x, present);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, d);
  if (lane == 0 && cnt) atomicAdd(&p.ctl->cnt_total, cnt);
}

template <typename T>
__global__ __launch_bounds__(MASK_WG) void k_mask_apply(MaskApplyParams<T> p) {
  const unsigned stride = gridDim.x * (unsigned)MASK_WG;
  for (unsigned o = blockIdx.x * (unsigned)MASK_WG + threadIdx.x; o < p.cnt; o += stride) {
    unsigned b[BOX_ND];
    const unsigned e = p.one_run ? p.first + o : p.box.flat_of(o, b);   // (wave-uniform choice) e < n: the box lies inside the array
    if ((p.mask32[e >> 5] >> (e & 31u)) & 1u) p.out[o] = p.fill;
  }
}

template <typename T>
void launch_mask_fill(const MaskFillParams<T>& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_fill<T>, dim3(grid), dim3(MASK_WG), 0, s, p);
}
template <typename T>
void launch_mask_apply(const MaskApplyParams<T>& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_apply<T>, dim3(grid), dim3(MASK_WG), 0, s, p);
}
template void launch_mask_fill<double>(const MaskFillParams<double>&, int, hipStream_t);
template void launch_mask_fill<float>(const MaskFillParams<float>&, int, hipStream_t);
template void launch_mask_apply<double>(const MaskApplyParams<double>&, int, hipStream_t);
template void launch_mask_apply<float>(const MaskApplyParams<float>&, int, hipStream_t);

}  // namespace dctz
