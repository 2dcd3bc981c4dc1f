// dct_lowband_block.h -- the LOW BAND of a block's inverse transform at reduced resolution, by one lane in registers
// (include/dctz_hip.h: dctzhip_decompress_coarse; every index a compile-time constant, as in dct64_block.h).
//
// A block of length N with de-quantised coefficients c[0 .. N-1] is reconstructed by the full decoder as
//     x[m] = sum_k alpha_N(k) c[k] cos(pi k (2m + 1) / (2N)),    alpha_N(0) = sqrt(1/N), alpha_N(k > 0) = sqrt(2/N).
// With K = N / f coefficients kept, the coarse decode writes K values
//     y[i] = sum_{k < K} alpha_N(k) c[k] cos(pi k (2i + 1) / (2K)),    i = 0 .. K-1:
// the part of x below frequency K at the centres of the K cells of f elements, i.e. the K-point orthonormal DCT-III of
// sqrt(K/N) c[0 .. K-1].  Its mean over the block is the block mean of x; K = 1 gives c[0] / sqrt(N).
//
// Flow: d[k] = alpha_N(k) c[k] (one multiply each), then an unnormalised K-point DCT-III by even / odd splitting,
//     y[i], y[K-1-i] = E[i] +- O[i],   E = the K/2-point DCT-III of d[0], d[2], ...,
//     O[i] = sum_j d[2j + 1] cos(pi (2j + 1)(2i + 1) / (2K))                    (a K/2 x K/2 matrix, mul + fma chain),
// down to K = 1: K^2 / 3 fused multiply-adds for K points, no scratch memory at K = 32.  All angles are multiples of
// pi / 64, so one table of 33 cosines serves every K; after unrolling each use is a literal constant.  Tiles (8 x 8,
// 4 x 4 x 4) run the same one-dimensional flow along every axis of their low corner k_a < K.
//
// The file compiles under hipcc (device + host) and under g++ (tests/emu/emu_lowband.cpp).
#pragma once
#include "dct64_block.h"

namespace dctz {

// cos(pi m / 64) for any integer m >= 0
template <typename T>
DCTZ_HD constexpr T lb_cos(int m) {
  constexpr double c[33] = {
      1.0, 0.9987954562051724, 0.9951847266721969, 0.989176509964781, 0.9807852804032304, 0.970031253194544,
      0.9569403357322088, 0.9415440651830208, 0.9238795325112867, 0.9039892931234433, 0.881921264348355, 0.8577286100002721,
      0.8314696123025452, 0.8032075314806449, 0.773010453362737, 0.7409511253549591, 0.7071067811865476, 0.6715589548470184,
      0.6343932841636455, 0.5956993044924334, 0.5555702330196022, 0.5141027441932218, 0.47139673682599764, 0.4275550934302821,
      0.3826834323650898, 0.33688985339222005, 0.2902846772544624, 0.2429801799032639, 0.19509032201612828, 0.14673047445536175,
      0.0980171403295606, 0.049067674327418015, 0.0};
  m &= 127;
  if (m > 64) m = 128 - m;
  return (T)(m > 32 ? -c[64 - m] : c[m]);
}

// alpha_N(0), alpha_N(k > 0) for the block lengths in use: 64 (flat), 8 (an axis of an 8 x 8 tile), 4 (of a 4 x 4 x 4 tile)
template <typename T, int N> struct LbAlpha;
template <typename T> struct LbAlpha<T, 64> { static constexpr T A0 = T(0.125), A1 = T(0.1767766952966369); };
template <typename T> struct LbAlpha<T, 8> { static constexpr T A0 = T(0.3535533905932738), A1 = T(0.5); };
template <typename T> struct LbAlpha<T, 4> { static constexpr T A0 = T(0.5), A1 = T(0.7071067811865476); };

// y[i] = sum_{k < K} d[k] cos(pi k (2i + 1) / (2K)), K a power of two up to 32
template <typename T, int K> struct LbDct3 {
  static_assert(K == 2 || K == 4 || K == 8 || K == 16 || K == 32, "K is a power of two in [1, 32]");
  static DCTZ_HD void run(const T (&d)[K], T (&y)[K]) {
    constexpr int H = K / 2;
    T e[H], E[H];
#pragma unroll
    for (int j = 0; j < H; j++) e[j] = d[2 * j];
    LbDct3<T, H>::run(e, E);
#pragma unroll
    for (int i = 0; i < H; i++) {
      T o = d[1] * lb_cos<T>((2 * i + 1) * (32 / K));
#pragma unroll
      for (int j = 1; j < H; j++) o = fma_(d[2 * j + 1], lb_cos<T>((2 * j + 1) * (2 * i + 1) * (32 / K)), o);
      y[i] = E[i] + o;
      y[K - 1 - i] = E[i] - o;
    }
  }
};
template <typename T> struct LbDct3<T, 1> {
  static DCTZ_HD void run(const T (&d)[1], T (&y)[1]) { y[0] = d[0]; }
};

// One block of length N: c[0 .. K-1] -> y[0 .. K-1] (not de-scaled: the caller multiplies by sf)
template <typename T, int N, int K>
DCTZ_HD void lowband_inv(const T (&c)[K], T (&y)[K]) {
  T d[K];
  d[0] = c[0] * LbAlpha<T, N>::A0;
#pragma unroll
  for (int k = 1; k < K; k++) d[k] = c[k] * LbAlpha<T, N>::A1;
  LbDct3<T, K>::run(d, y);
}

// The low corner of an 8 x 8 tile, v[ky * K + kx] -> y[iy * K + ix], K = 2 | 4: rows, then columns
template <typename T, int K>
DCTZ_HD void lowband_inv_2d(T (&v)[K * K]) {
  T a[K], b[K];
#pragma unroll
  for (int r = 0; r < K; r++) {
#pragma unroll
    for (int i = 0; i < K; i++) a[i] = v[r * K + i];
    lowband_inv<T, 8, K>(a, b);
#pragma unroll
    for (int i = 0; i < K; i++) v[r * K + i] = b[i];
  }
#pragma unroll
  for (int q = 0; q < K; q++) {
#pragma unroll
    for (int i = 0; i < K; i++) a[i] = v[i * K + q];
    lowband_inv<T, 8, K>(a, b);
#pragma unroll
    for (int i = 0; i < K; i++) v[i * K + q] = b[i];
  }
}

// The low corner of a 4 x 4 x 4 tile, v[(kz * K + ky) * K + kx], K = 2: along x, then y, then z
template <typename T, int K>
DCTZ_HD void lowband_inv_3d(T (&v)[K * K * K]) {
  T a[K], b[K];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const int st = ax == 0 ? 1 : (ax == 1 ? K : K * K);                // stride of the axis transformed
#pragma unroll
    for (int r = 0; r < K * K; r++) {
      // the r-th line along the axis: the other two coordinates (u slower, w faster)
      const int u = r / K, w = r % K;
      const int base = ax == 0 ? (u * K + w) * K : (ax == 1 ? u * K * K + w : u * K + w);
#pragma unroll
      for (int i = 0; i < K; i++) a[i] = v[base + i * st];
      lowband_inv<T, 4, K>(a, b);
#pragma unroll
      for (int i = 0; i < K; i++) v[base + i * st] = b[i];
    }
  }
}

}  // namespace dctz
