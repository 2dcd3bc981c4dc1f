// dctz_kernels_ndrd.hip -- the rate-distortion probe of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (include/dctz_hip.h:
// dctzhip_rd_probe_nd).  ONE read of the array in place: every tile is scaled and transformed once, as
// dctzhip_compress_nd does it, and binned against up to RD_MAXK error bounds in registers.  Everything behind the block
// transform is the flat probe's (dctz_rd_coef.h, the slab rows, k_rd_final); three things are this file's.
//
//   * The lane's block comes straight out of the array: block B of the row-major tile grid (ndfix_block), 8 rows of 8 or 16
//     rows of 4, a coordinate beyond an extent clamped to the axis' last sample (nd_locate's rule in k_gather_nd).  Where the
//     fastest extent is a multiple of a 16-byte vector's elements every in-block row is whole vectors, each inside the array
//     or all padding; otherwise the elements are loaded one by one.  Nothing is read beyond the array.
//   * The separable transform, block_fwd<GEOM>.
//   * The padded share.  Orthonormality gives the squared error over all 64 places of a block; in a tile that hangs over an
//     extent some of those are padding and no part of the array.  By linearity the reconstruction's error at place j is
//     sf * (inverse transform of the coefficient errors c - c^)[j] up to rounding, so for the blocks with padding -- the
//     last tile row / column / slab of a ragged axis, a surface enumerated arithmetically -- k_ndrd_edge repeats load, scale
//     and transform, forms the 64 coefficient errors of every bound, runs block_inv<GEOM> on them and leaves the NEGATED sum
//     of the squares at the padded places in slab rows of its own behind k_ndrd_probe's (zero counts, neutral min / max), as
//     k_rd_probe_rem leaves its row.  k_rd_final adds all rows in index order: bitwise reproducible, and a bound's result
//     does not depend on the others.  The counts are k_ndrd_probe's alone: the streams do carry the padded coefficients.
//
// (Not named k_rd_probe...: the flat family's budget test counts every kernel of that name.)
#include "dctz_nd_image.h"
#include "dctz_rd_coef.h"

namespace dctz {

// Block (bz, by, bx) of the tile grid into x[], in-block place j at x[j]
template <typename T, int GEOM>
__device__ __forceinline__ void ndrd_load(const NdRdParams<T>& p, const unsigned bz, const unsigned by, const unsigned bx, T (&x)[64]) {
  using Vec = typename Traits<T>::Vec;
  constexpr int EPV = Traits<T>::EPV;
  constexpr unsigned E = GEOM == GEOM_2D ? 8u : 4u;
  constexpr int ROWS = 64 / (int)E;
  const unsigned dx = p.d[2], dy = p.d[1], dz = p.d[0];
#pragma unroll
  for (int r = 0; r < ROWS; r++) {
    const unsigned z = GEOM == GEOM_3D ? min(bz * 4u + (unsigned)(r >> 2), dz - 1u) : 0u;
    const unsigned y = GEOM == GEOM_3D ? min(by * 4u + (unsigned)(r & 3), dy - 1u) : min(by * 8u + (unsigned)r, dy - 1u);
    const T* const row = p.rd.x + ((size_t)z * dy + y) * dx;
    if (p.vec) {
#pragma unroll
      for (int v = 0; v < (int)E / EPV; v++) {
        const unsigned c0 = bx * E + (unsigned)(v * EPV);
        const bool in = c0 < dx;                               // (dx is whole vectors: inside the row, or all padding)
        T e[EPV];
        Traits<T>::unpack(load_stream(reinterpret_cast<const Vec*>(row + (in ? c0 : dx - (unsigned)EPV))), e);
#pragma unroll
        for (int i = 0; i < EPV; i++) x[r * (int)E + v * EPV + i] = in ? e[i] : e[EPV - 1];
      }
    } else {
#pragma unroll
      for (int cc = 0; cc < (int)E; cc++) x[r * (int)E + cc] = row[min(bx * E + (unsigned)cc, dx - 1u)];
    }
  }
}

// x / sf as k_compress scales (stats_scale), then the block transform
template <typename T, int GEOM>
__device__ __forceinline__ void ndrd_scale_fwd(T (&x)[64], const bool scale, const unsigned fast_sf, const FastDiv<T>& sfd, const CTab<T> tab) {
  if (scale) {                                           // dctz-comp-lib.c:197-199 / :212-214
    if (fast_sf == 2) {
#pragma unroll
      for (int j = 0; j < 64; j++) x[j] = sfd.core(x[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 64; j++) x[j] = x[j] / sfd.d;         // (fast_sf 1, FastDiv::div: the same quotient)
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  block_fwd<T, CTab<T>, GEOM, (sizeof(T) == 8)>(x, tab);
  __builtin_amdgcn_sched_barrier(0);
}

// One pass over all tiles.  Wave w of workgroup g takes stream tiles g * NW + w, then every gridDim.x * NW-th; lane b block b.
template <typename T, int GEOM>
__global__ __launch_bounds__(RD_WG) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 8 ? 1 : 2, sizeof(T) == 8 ? 1 : 2))) void k_ndrd_probe(NdRdParams<T> p) {
  constexpr int NW = RD_WG / 64;
  __shared__ double s_e[NW][RD_MAXK];
  __shared__ unsigned long long s_c[NW][RD_MAXK];
  __shared__ double s_mm[2][NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < RD_MAXK) { s_e[wave][lane] = 0.0; s_c[wave][lane] = 0ull; }
  const T sf = p.rd.sf;
  const bool scale = (sf != T(1));                       // dctz-comp-lib.c:193 / :208
  FastDiv<T> sfd;
  sfd.init(sf, p.rd.fast_sf != 0);
  const CTab<T> tab = as_ctab<T>(p.rd.tab);
  const CTab<T> bc = as_ctab<T>(p.rd.bounds);
  double mn = 1.79769313486231570815e308, mx = -1.79769313486231570815e308;
  const unsigned nblk = p.rd.nfull;
  const unsigned ntiles = (nblk + TILE_BLKS - 1) / TILE_BLKS;
  for (unsigned tile = blockIdx.x * NW + wave; tile < ntiles; tile += gridDim.x * NW) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    const unsigned blk = tile * TILE_BLKS + (unsigned)lane;
    const bool active = blk < nblk;
    unsigned bz, by, bx;
    ndfix_block<GEOM>(active ? blk : 0u, p.nb[2], p.nb[1], bz, by, bx);
    T x[64];
    ndrd_load<T, GEOM>(p, bz, by, bx, x);
    if (active) {                                        // (a repeated edge sample changes neither)
#pragma unroll
      for (int j = 0; j < 64; j++) { mn = fmin(mn, (double)x[j]); mx = fmax(mx, (double)x[j]); }
    }
    ndrd_scale_fwd<T, GEOM>(x, scale, p.rd.fast_sf, sfd, tab);
    const double e_dc = rd_dc_err2<T>(x[0]);
    for (int kk = 0; kk < p.rd.k; kk++) {
      // (the coefficients are "changed" here, so that nothing bound-independent is hoisted out of this loop, as in k_rd_probe)
#pragma unroll
      for (int j = 0; j < 64; j++) asm volatile("" : "+v"(x[j]));
      const T rmin = bc[3 * kk], rmax = bc[3 * kk + 1], bw = bc[3 * kk + 2];
      const bool fast = ((p.rd.fast_bw >> kk) & 1u) != 0u;
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
  double* row = p.rd.slab + (size_t)blockIdx.x * RD_SLOT;
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) { mn = fmin(mn, s_mm[0][w]); mx = fmax(mx, s_mm[1][w]); }
    row[0] = mn; row[1] = mx;
  }
  if ((int)threadIdx.x < p.rd.k) {
    const int kk = threadIdx.x;
    double e = s_e[0][kk];
    unsigned long long c = s_c[0][kk];
    for (int w = 1; w < NW; w++) { e += s_e[w][kk]; c += s_c[w][kk]; }
    row[2 + 2 * kk] = e;
    row[3 + 2 * kk] = __longlong_as_double((long long)c);
  }
}

// Edge block number e of p.nedge -> its grid coordinates: first the last slab of a ragged z (every by, bx), then the last
// tile row of a ragged y (the z left over, every bx), then the last column of a ragged x (the z and y left over).
__device__ __forceinline__ void ndrd_edge_block(const unsigned (&nb)[3], const unsigned (&rag)[3], unsigned e, unsigned& bz, unsigned& by, unsigned& bx) {
  const unsigned nbz = nb[0], nby = nb[1], nbx = nb[2];
  const unsigned fz = rag[0] ? nby * nbx : 0u;
  if (e < fz) { bz = nbz - 1u; by = e / nbx; bx = e - by * nbx; return; }
  e -= fz;
  const unsigned mz = nbz - rag[0];
  const unsigned fy = rag[1] ? mz * nbx : 0u;
  if (e < fy) { by = nby - 1u; bz = e / nbx; bx = e - bz * nbx; return; }
  e -= fy;
  const unsigned my = nby - rag[1];
  bx = nbx - 1u; bz = e / my; by = e - bz * my;
}

// The padded share of every bound's sum, negated (see the top of the file).  One wave a workgroup, lane b edge block 64 t + b
// of edge tile t = blockIdx.x, then every gridDim.x-th; workgroup g leaves slab row p.edge_row + g.
template <typename T, int GEOM>
__global__ __launch_bounds__(64) void k_ndrd_edge(NdRdParams<T> p) {
  __shared__ double s_e[RD_MAXK];
  const int lane = threadIdx.x;
  if (lane < RD_MAXK) s_e[lane] = 0.0;
  const T sf = p.rd.sf;
  const bool scale = (sf != T(1));
  FastDiv<T> sfd;
  sfd.init(sf, p.rd.fast_sf != 0);
  const CTab<T> tab = as_ctab<T>(p.rd.tab);
  const CTab<T> bc = as_ctab<T>(p.rd.bounds);
  const unsigned ntiles = (p.nedge + TILE_BLKS - 1) / TILE_BLKS;
  for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    asm volatile("" ::: "memory");
    const unsigned e = tile * TILE_BLKS + (unsigned)lane;
    const bool active = e < p.nedge;
    unsigned bz, by, bx;
    ndrd_edge_block(p.nb, p.rag, active ? e : 0u, bz, by, bx);
    const unsigned long long pad = active ? ~nd_real_mask<GEOM>(bz, by, bx, p.d[0], p.d[1], p.d[2]) : 0ull;
    T x[64];
    ndrd_load<T, GEOM>(p, bz, by, bx, x);
    ndrd_scale_fwd<T, GEOM>(x, scale, p.rd.fast_sf, sfd, tab);
    for (int kk = 0; kk < p.rd.k; kk++) {
#pragma unroll
      for (int j = 0; j < 64; j++) asm volatile("" : "+v"(x[j]));
      const T rmin = bc[3 * kk], rmax = bc[3 * kk + 1], bw = bc[3 * kk + 2];
      const bool fast = ((p.rd.fast_bw >> kk) & 1u) != 0u;
      FastDiv<T> bwd;
      bwd.init(bw, fast);
      T err[64];
      err[0] = x[0] - (T)(float)x[0];                         // :350-351 USE_TRUNCATE
#pragma unroll
      for (int j = 1; j < 64; j++) {
        bool ex;
        err[j] = x[j] - rd_value<T>(x[j], rmin, rmax, bw, bwd, fast, ex);
        if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      block_inv<T, CTab<T>, GEOM, (sizeof(T) == 4)>(err, tab);
      __builtin_amdgcn_sched_barrier(0);
      double e2 = 0.0;
#pragma unroll
      for (int j = 0; j < 64; j++) {
        const double d = (double)err[j];
        e2 = ((pad >> j) & 1ull) ? __builtin_fma(d, d, e2) : e2;
      }
      unsigned none = 0u;
      rd_wave_sum(e2, none);
      if (lane == 0) s_e[kk] += e2;
    }
  }
  __syncthreads();
  double* row = p.rd.slab + (size_t)(p.edge_row + blockIdx.x) * RD_SLOT;
  if (lane == 0) { row[0] = 1.79769313486231570815e308; row[1] = -1.79769313486231570815e308; }
  if (lane < p.rd.k) {
    row[2 + 2 * lane] = -s_e[lane];
    row[3 + 2 * lane] = __longlong_as_double(0ll);
  }
}

template <typename T>
void launch_ndrd_probe(const NdRdParams<T>& p, int geom, int grid, int edge_grid, hipStream_t s) {
  if (geom == GEOM_3D) {
    hipLaunchKernelGGL((k_ndrd_probe<T, GEOM_3D>), dim3(grid), dim3(RD_WG), 0, s, p);
    if (edge_grid > 0) hipLaunchKernelGGL((k_ndrd_edge<T, GEOM_3D>), dim3(edge_grid), dim3(64), 0, s, p);
  } else {
    hipLaunchKernelGGL((k_ndrd_probe<T, GEOM_2D>), dim3(grid), dim3(RD_WG), 0, s, p);
    if (edge_grid > 0) hipLaunchKernelGGL((k_ndrd_edge<T, GEOM_2D>), dim3(edge_grid), dim3(64), 0, s, p);
  }
  launch_rd_final(p.rd.slab, (unsigned)(grid + edge_grid), p.rd.out, p.rd.k, s);
}
template void launch_ndrd_probe<double>(const NdRdParams<double>&, int, int, int, hipStream_t);
template void launch_ndrd_probe<float>(const NdRdParams<float>&, int, int, int, hipStream_t);

}  // namespace dctz
