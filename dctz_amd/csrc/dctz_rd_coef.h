// dctz_rd_coef.h -- what the rate-distortion probes do to one coefficient and one bound, and the wave's fixed shuffle tree
// (dctz_kernels_rd.hip: flat blocks; dctz_kernels_ndrd.hip: 8 x 8 / 4 x 4 x 4 tiles).  The derivation is at the top of
// dctz_kernels_rd.hip and in DESIGN.md section 12.
#pragma once
#include "dctz_kernel_common.h"

namespace dctz {

__device__ __forceinline__ void rd_wave_sum(double& e, unsigned& c) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    e += __shfl_xor(e, d);
    c += __shfl_xor(c, d);
  }
}

// The decoder's value for the scaled, transformed coefficient `x` at a position j >= 1 under one bound; ex: stored exactly.
template <typename T>
__device__ __forceinline__ T rd_value(T x, T rmin, T rmax, T bw, const FastDiv<T>& bwd, bool fast, bool& ex) {
  const T u = x - rmin;                                   // dctz-comp-lib.c:377 / :402
  const T q = fast ? bwd.core(u) : u / bwd.d;             // (k_compress makes the same choice, per launch)
  const float h = bin_value<T, true>(x, q, rmax);
  ex = h >= 255.0f;                                       // v_cvt_pk_u8_f32 saturates this to 255: stored exactly
  const T centre = (floor(q) - T(127)) * bw;              // the decoder's bin centre (see the top of dctz_kernels_rd.hip)
  return ex ? (T)(float)x : centre;
}

// The work of one bound on one coefficient at position j >= 1.  `x` is the scaled, transformed coefficient.
template <typename T>
__device__ __forceinline__ void rd_coef(T x, T rmin, T rmax, T bw, const FastDiv<T>& bwd, bool fast, double& e2, unsigned& c) {
  bool ex;
  const T r = rd_value<T>(x, rmin, rmax, bw, bwd, fast, ex);
  const double d = (double)x - (double)r;
  e2 = __builtin_fma(d, d, e2);
  c += ex ? 1u : 0u;
}

template <typename T>
__device__ __forceinline__ double rd_dc_err2(T c0) {
  const double d = (double)c0 - (double)(float)c0;        // :350-351 USE_TRUNCATE
  return d * d;
}

}  // namespace dctz
