// The quantiser's launch constants (host only: plain C++, no HIP): the numbers that decide which bin a coefficient lands in
// and which division a kernel runs.  Each is a handful of casts whose ORDER matters to the last bit of the streams, so each
// is written here once, for every path that fills a parameter block.  Two forms, on purpose: on compress the reference
// computes the ranges in double and stores them in the element type (dctz-comp-lib.c:271-281); on decode gen_bins_f
// receives the bound ALREADY rounded to float (binning.c:17 / :37) and the ranges are dctz-decomp-lib.c:372-381.  The two
// round eb at different points; neither is to be rewritten as the other, even where the values coincide.
#pragma once
#include <cmath>
#include "../../include/dctz_hip.h"
#include "dctz_tables.h"

namespace dctz {

// FastDiv's divisor window (dctz_kernels.hip): |d| in [2^-250, 2^250] (f64) / [2^-30, 2^30] (f32)
inline unsigned divisor_in_window(int dtype, double d) {
  if (!(d == d) || d == 0.0 || std::isinf(d)) return 0;      // (inf: sf of an array that holds an infinity; frexp says nothing about it)
  int e = 0;
  (void)frexp(fabs(d), &e);                      // |d| = m * 2^e, m in [0.5, 1)
  return (dtype == DCTZHIP_F64) ? (e - 1 >= -250 && e - 1 < 250) : (e - 1 >= -30 && e - 1 < 30);
}

// FastDiv's numerator window: |x| in [2^-500, 2^500] (f64) / [2^-63, 2^63] (f32), zero excluded
inline bool value_in_window(int dtype, double v) {
  if (!(v == v) || v == 0.0 || std::isinf(v)) return false;
  int e = 0;
  (void)frexp(fabs(v), &e);
  return (dtype == DCTZHIP_F64) ? (e - 1 >= -500 && e - 1 < 500) : (e - 1 >= -63 && e - 1 < 63);
}

template <typename T> struct FwdQuant { T bin_width, range_min, range_max; unsigned fast_bw; };
template <typename T> struct InvQuant { T bin_width, range_min, range_max; };

// Compress: the bin ranges (computed in double, stored in T) and FwdParams::fast_bw for them under DCTZHIP_FASTDIV = fastdiv
// (bit 0: the bin width is in FastDiv's divisor window)
template <typename T>
inline FwdQuant<T> fwd_quant(double eb, int fastdiv) {
  const int half = DCTZHIP_NBINS / 2;
  FwdQuant<T> r;
  r.bin_width = (T)(eb * 2.0 * 1.0);
  r.range_min = (T)(-(half * 2 + 1) * (eb * 1.0));
  r.range_max = (T)((half * 2 + 1) * (eb * 1.0));
  r.fast_bw = fastdiv ? divisor_in_window(sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32, (double)r.bin_width) : 0u;      // bit 0
  // bit 1: "item > range_max  =>  (item - range_min) / bin_width >= 255" holds for these launch constants, in T
  // arithmetic, so k_compress needs no separate range test (dctz_kernels.hip, bin_value): the smallest such
  // numerator is fl(range_max - range_min) = 2 range_max, and rounding is monotonic.
  volatile T u = (T)(r.range_max - r.range_min);
  volatile T q = (T)(u / r.bin_width);
  if (r.fast_bw && fastdiv >= 2 && q >= (T)255) r.fast_bw |= 2u;
  return r;
}

// Decode: bin_width = error_bound*2*BRSF in the data type, from the bound rounded to it first; the ranges from the double
template <typename T>
inline InvQuant<T> inv_quant(double eb) {
  return {(T)((T)eb * 2 * 1.0), (T)(-eb * DCTZHIP_NBINS), (T)(eb * DCTZHIP_NBINS)};      // bin_width, range_min, range_max
}

// FwdParams::fast_sf for a scaling factor (as rounded to the element type) and the array's statistics.  0: plain division;
// 1: FastDiv with a window test per element; 2: min|x| and max|x|, so every element, are inside FastDiv's numerator
// window -> no per-element test.  Never 2 on placeholder statistics (the device chooses sf and its level itself).
inline unsigned fast_sf_level(int dtype, int fastdiv, double sf_in_T, double min_abs, double max_abs, bool stats_are_true) {
  if (!fastdiv || !divisor_in_window(dtype, sf_in_T)) return 0u;
  return (stats_are_true && fastdiv >= 2 && value_in_window(dtype, min_abs) && value_in_window(dtype, max_abs)) ? 2u : 1u;
}

// The verdict on a scaling factor the DEVICE chose (sf_used, at division level fast_used): the host's own expression on the
// true statistics equals it in the element type, and level 2 only if min and max are in the value window.
inline bool device_sf_stands(int dtype, double max_abs, double min_abs, double sf_used, unsigned fast_used, double* true_sf) {
  *true_sf = scaling_factor(dtype, max_abs);
  const bool same = dtype == DCTZHIP_F64 ? *true_sf == sf_used : (float)*true_sf == (float)sf_used;
  const bool window_ok = fast_used != 2 || (value_in_window(dtype, min_abs) && value_in_window(dtype, max_abs));
  return same && window_ok;
}

}  // namespace dctz
