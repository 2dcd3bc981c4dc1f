// dctz_mask_fill.h -- the fill rule of the missing-value layer inside one block, shared by k_mask_fill (a block is 64
// consecutive elements) and k_ndmask_fill (a block is an 8 x 8 / 4 x 4 x 4 tile): include/dctz_hip.h, DESIGN section 13.
//
// A lane holds 16 bytes, E = 2 fp64 or 4 fp32 elements, as bit patterns; the L = 64 / E lanes of a block are neighbours in
// the wave and stand in block order, whatever addresses their elements came from.  Nothing here reads or writes memory but
// mask_store_lane, which writes the lane's own elements.
#pragma once
#include "dctz_kernel_common.h"

namespace dctz {

template <typename T> struct MaskBits { using U = unsigned long long; };
template <> struct MaskBits<float> { using U = unsigned; };

template <typename T>
__device__ __forceinline__ bool mask_is_missing(const T v, const unsigned flags, const T value, const T limit) {
  return ((flags & DCTZHIP_MISS_NAN) && v != v) || ((flags & DCTZHIP_MISS_INF) && fabs(v) == (T)INFINITY) ||
         ((flags & DCTZHIP_MISS_VALUE) && v == value) || ((flags & DCTZHIP_MISS_ABS_GE) && fabs(v) >= limit);
}

// The lane settles its own elements: bit k of the result = element k is there (`present`) and missing.
template <typename T>
__device__ __forceinline__ unsigned mask_settle(const typename MaskBits<T>::U (&x)[16 / sizeof(T)], const unsigned present, const unsigned flags,
                                                const T value, const T limit) {
  constexpr int E = 16 / (int)sizeof(T);
  unsigned miss = 0;
#pragma unroll
  for (int k = 0; k < E; k++) miss |= mask_is_missing<T>(__builtin_bit_cast(T, x[k]), flags, value, limit) ? 1u << k : 0u;
  return miss & present;
}

// The fill: every element of x without a bit in `valid` takes the nearest valid element in front of it in the lane's block,
// else the block's first valid one, else +0.0.  The whole wave calls this together.
template <typename T>
__device__ __forceinline__ void mask_fill_block(typename MaskBits<T>::U (&x)[16 / sizeof(T)], const unsigned valid, const int lane) {
  using U = typename MaskBits<T>::U;
  constexpr int E = 16 / (int)sizeof(T);             // elements of a lane
  constexpr int L = 64 / E;                          // lanes of a block
  // the nearest lane in front that holds a valid element of this block hands over its last one; with none in front, the
  // block's first lane that holds one -- this lane itself or one behind it -- hands over its first one
  const unsigned long long has = __ballot(valid != 0u) & (((1ull << L) - 1ull) << (lane & ~(L - 1)));
  U lastv = U(0), firstv = U(0);
#pragma unroll
  for (int k = 0; k < E; k++) lastv = (valid >> k) & 1u ? x[k] : lastv;
#pragma unroll
  for (int k = E - 1; k >= 0; k--) firstv = (valid >> k) & 1u ? x[k] : firstv;
  const unsigned long long front = has & ((1ull << lane) - 1ull);
  const U from_front = __shfl(lastv, front ? 63 - __clzll((long long)front) : lane);
  const U from_first = __shfl(firstv, has ? __ffsll((unsigned long long)has) - 1 : lane);
  U run = front ? from_front : has ? from_first : U(0);   // (no valid element in the block: +0.0)
#pragma unroll
  for (int k = 0; k < E; k++) {
    if ((valid >> k) & 1u) run = x[k];
    else x[k] = run;
  }
}

// The lane's elements to out[e0 ...]: 16 bytes at once where `whole` says all are there (and out + e0 is 16-byte aligned),
// else those of `present` one by one.
template <typename T>
__device__ __forceinline__ void mask_store_lane(typename MaskBits<T>::U* const out, const unsigned e0,const typename MaskBits<T>::U (&x)[16 / sizeof(T)],
                                                const unsigned present, const bool whole) {
  constexpr int E = 16 / (int)sizeof(T);
  if (whole) {
    u32x4 v;
    __builtin_memcpy(&v, x, 16);
    *reinterpret_cast<u32x4*>(out + e0) = v;
  } else {
#pragma unroll
    for (int k = 0; k < E; k++) if ((present >> k) & 1u) out[e0 + k] = x[k];
  }
}

}  // namespace dctz
