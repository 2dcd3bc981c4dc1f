// dctz_kernels_rd.hip -- the rate-distortion probe (include/dctz_hip.h: dctzhip_rd_probe): ONE read of an array, every
// block scaled and transformed once, exactly as k_compress does it, then binned against up to RD_MAXK error bounds in
// registers.  For every bound it yields the exact tot_AC_exact_count and the predicted squared error of the
// reconstruction, without encoding or decoding anything.
//
// Why the prediction holds: the 64-point DCT-II of the reference is orthonormal, so the squared
// error of a reconstructed block is the sum of its coefficients' squared errors (times sf^2 after the de-scaling), up to
// the rounding of the inverse transform.  Each coefficient's error is known the moment it is binned, because the
// decoder's value for it is fixed by the stream:
//   * in range, bin f = floor((c - range_min) / bin_width):  the decoder's centre bin_center[conv_tbl_i[b]] (binning.c:
//     17-23) is (T)(f - 127) * bin_width  (both branches of conv_tbl, dctz-comp-lib.c:27-43, give the same m = f - 127);
//   * stored exactly (bin 255, USE_TRUNCATE):  (T)(float)c;
//   * DC (position 0):  (T)(float)c0.
// The count of exact coefficients is the reference's own tot_AC_exact_count (positions j >= 1 with bin 255).
//
// Work decomposition: a wavefront takes a TILE of 64 blocks at a time, lane b block b of it, and reads its 64 values
// straight from HBM (the probe is arithmetic-bound: ~14 fp64 operations per coefficient and bound against ~0.5 for the
// load).  The bound loop runs OUTSIDE the coefficient loop, so one bound's accumulators are live at a time; after each
// bound of each tile the wave's sums go through a fixed shuffle tree into the wave's own LDS slot.  Workgroups leave
// one slab row each, and k_rd_final adds the rows up in index order: the results are bitwise reproducible, no float
// atomics anywhere.  The short last block (n % 64) is k_rd_probe_rem's, as k_compress_rem's is on compress.
#include "dctz_rd_coef.h"

namespace dctz {

// One pass over the whole blocks.  Wave w of workgroup g takes tiles g * NW + w, then every gridDim.x * NW-th.
template <typename T>
__global__ __launch_bounds__(RD_WG) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 8 ? 1 : 2, sizeof(T) == 8 ? 1 : 2))) void k_rd_probe(RdParams<T> p) {
  constexpr int NW = RD_WG / 64;
  __shared__ double s_e[NW][RD_MAXK];
  __shared__ unsigned long long s_c[NW][RD_MAXK];
  __shared__ double s_mm[2][NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < RD_MAXK) { s_e[wave][lane] = 0.0; s_c[wave][lane] = 0ull; }
  const T sf = p.sf;
  const bool scale = (sf != T(1));                       // dctz-comp-lib.c:193 / :208
  FastDiv<T> sfd;
  sfd.init(sf, p.fast_sf != 0);
  const CTab<T> tab = as_ctab<T>(p.tab);
  const CTab<T> bc = as_ctab<T>(p.bounds);
  double mn = 1.79769313486231570815e308, mx = -1.79769313486231570815e308;
  const unsigned ntiles = (p.nfull + TILE_BLKS - 1) / TILE_BLKS;
  using Vec = typename Traits<T>::Vec;
  constexpr int EPV = Traits<T>::EPV;
  for (unsigned tile = blockIdx.x * NW + wave; tile < ntiles; tile += gridDim.x * NW) {
    // (a compiler barrier per trip: the transform's constants are loop-invariant scalar loads, and hoisted out of the tile
    // loop all 532 of them are live at once -- hundreds of spilled SGPRs)
    asm volatile("" ::: "memory");
    const unsigned blk = tile * TILE_BLKS + (unsigned)lane;
    const bool active = blk < p.nfull;
    T x[64];
    const Vec* src = reinterpret_cast<const Vec*>(p.x + (size_t)(active ? blk : 0u) * 64);
#pragma unroll
    for (int v = 0; v < 64 / EPV; v++) Traits<T>::unpack(load_stream(src + v), &x[v * EPV]);
    if (active) {
#pragma unroll
      for (int j = 0; j < 64; j++) { mn = fmin(mn, (double)x[j]); mx = fmax(mx, (double)x[j]); }
    }
    if (scale) {                                         // dctz-comp-lib.c:197-199 / :212-214, as k_compress scales (stats_scale)
      if (p.fast_sf == 2) {
#pragma unroll
        for (int j = 0; j < 64; j++) x[j] = sfd.core(x[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 64; j++) x[j] = x[j] / sfd.d;       // (fast_sf 1, FastDiv::div: the same quotient, test_fast_division_is_exact)
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    block_fwd<T, CTab<T>, GEOM_1D, (sizeof(T) == 8)>(x, tab);
    __builtin_amdgcn_sched_barrier(0);
    const double e_dc = rd_dc_err2<T>(x[0]);
    for (int kk = 0; kk < p.k; kk++) {
      // (the coefficients are "changed" here, so that nothing bound-independent -- the float truncation of every
      // coefficient -- is hoisted out of this loop: 64 more live registers)
#pragma unroll
      for (int j = 0; j < 64; j++) asm volatile("" : "+v"(x[j]));
      const T rmin = bc[3 * kk], rmax = bc[3 * kk + 1], bw = bc[3 * kk + 2];
      const bool fast = ((p.fast_bw >> kk) & 1u) != 0u;
      FastDiv<T> bwd;
      bwd.init(bw, fast);
      double e2 = e_dc;
      unsigned c = 0;
#pragma unroll
      for (int j = 1; j < 64; j++) {
        rd_coef<T>(x[j], rmin, rmax, bw, bwd, fast, e2, c);
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // groups of four chains (all 63 at once: registers)
      }
      if (!active) { e2 = 0.0; c = 0u; }
      rd_wave_sum(e2, c);
      if (lane == 0) { s_e[wave][kk] += e2; s_c[wave][kk] += c; }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { mn = fmin(mn, __shfl_xor(mn, d)); mx = fmax(mx, __shfl_xor(mx, d)); }
  if (lane == 0) { s_mm[0][wave] = mn; s_mm[1][wave] = mx; }
  __syncthreads();
  double* row = p.slab + (size_t)blockIdx.x * RD_SLOT;
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) { mn = fmin(mn, s_mm[0][w]); mx = fmax(mx, s_mm[1][w]); }
    row[0] = mn; row[1] = mx;
  }
  if ((int)threadIdx.x < p.k) {
    const int kk = threadIdx.x;
    double e = s_e[0][kk];
    unsigned long long c = s_c[0][kk];
    for (int w = 1; w < NW; w++) { e += s_e[w][kk]; c += s_c[w][kk]; }
    row[2 + 2 * kk] = e;
    row[3 + 2 * kk] = __longlong_as_double((long long)c);
  }
}

// The last, short block (length l = n % 64): scaled and transformed as k_compress_rem does it (dctz_kernels.hip:
// compress_rem_body -- the reference re-plans a length-l / 2l FFT, dctz-comp-lib.c:326-336, dct.c:59-72; there and here
// the same definition-order DFT with the same host-built roots), one coefficient per lane, then every bound.
template <typename T>
__global__ __launch_bounds__(64) void k_rd_probe_rem(RdParams<T> p, int l, unsigned row_at) {
  __shared__ T v[128];
  const int k = threadIdx.x;
  const size_t base = (size_t)p.nfull * 64;
  const T sf = p.sf;
  const bool SCALE = (sf != T(1));
  FastDiv<T> sfd;
  sfd.init(sf, p.fast_sf != 0);
  double mn = 1.79769313486231570815e308, mx = -1.79769313486231570815e308;
  if (k < l) {
    T a = p.x[base + k];
    mn = (double)a; mx = (double)a;
    if (SCALE) a = sfd.div(a);
    short_fwd_fill(v, l, k, a);
  }
  __syncthreads();
  T coef = T(0);
  if (k < l) coef = short_fwd_sum(v, p.rtab, short_dft_len(l), k);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { mn = fmin(mn, __shfl_xor(mn, d)); mx = fmax(mx, __shfl_xor(mx, d)); }
  double* row = p.slab + (size_t)row_at * RD_SLOT;
  if (k == 0) { row[0] = mn; row[1] = mx; }
  for (int kk = 0; kk < p.k; kk++) {
    const T rmin = p.bounds[3 * kk], rmax = p.bounds[3 * kk + 1], bw = p.bounds[3 * kk + 2];
    const bool fast = ((p.fast_bw >> kk) & 1u) != 0u;
    FastDiv<T> bwd;
    bwd.init(bw, fast);
    double e2 = 0.0;
    unsigned c = 0;
    if (k == 0) e2 = rd_dc_err2<T>(coef);
    else if (k < l) rd_coef<T>(coef, rmin, rmax, bw, bwd, fast, e2, c);
    rd_wave_sum(e2, c);
    if (k == 0) { row[2 + 2 * kk] = e2; row[3 + 2 * kk] = __longlong_as_double((long long)(unsigned long long)c); }
  }
}

// Rows [0, nrows) of the slab -> out[0 .. 2 + 2k): workgroup q adds up column q over the rows in a fixed order (strided
// per thread, then a fixed tree): min x, max x, then per bound the error sum and the count.
__global__ __launch_bounds__(SWG) void k_rd_final(const double* __restrict__ slab, unsigned nrows, double* __restrict__ out) {
  const int q = blockIdx.x;
  const bool is_min = q == 0, is_max = q == 1, is_cnt = q >= 2 && (q & 1);
  double a = is_min ? 1.79769313486231570815e308 : is_max ? -1.79769313486231570815e308 : 0.0;
  unsigned long long n = 0;
  for (unsigned r = threadIdx.x; r < nrows; r += SWG) {
    const double v = slab[(size_t)r * RD_SLOT + q];
    if (is_min) a = fmin(a, v);
    else if (is_max) a = fmax(a, v);
    else if (is_cnt) n += (unsigned long long)__double_as_longlong(v);
    else a += v;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const double b = __shfl_xor(a, d);
    a = is_min ? fmin(a, b) : is_max ? fmax(a, b) : a + b;
    n += __shfl_xor(n, d);
  }
  __shared__ double s_a[SWG / 64];
  __shared__ unsigned long long s_n[SWG / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_a[wave] = a; s_n[wave] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SWG / 64; w++) { a = is_min ? fmin(a, s_a[w]) : is_max ? fmax(a, s_a[w]) : a + s_a[w]; n += s_n[w]; }
    out[q] = is_cnt ? __longlong_as_double((long long)n) : a;
  }
}

void launch_rd_final(const double* slab, unsigned nrows, double* out, int k, hipStream_t s) {
  hipLaunchKernelGGL(k_rd_final, dim3(2 + 2 * k), dim3(SWG), 0, s, slab, nrows, out);
}

template <typename T>
void launch_rd_probe(const RdParams<T>& p, int grid, int rem, hipStream_t s) {
  if (grid > 0) hipLaunchKernelGGL(k_rd_probe<T>, dim3(grid), dim3(RD_WG), 0, s, p);
  if (rem) hipLaunchKernelGGL(k_rd_probe_rem<T>, dim3(1), dim3(64), 0, s, p, rem, (unsigned)grid);
  launch_rd_final(p.slab, (unsigned)grid + (rem ? 1u : 0u), p.out, p.k, s);
}
template void launch_rd_probe<double>(const RdParams<double>&, int, int, hipStream_t);
template void launch_rd_probe<float>(const RdParams<float>&, int, int, hipStream_t);

}  // namespace dctz
