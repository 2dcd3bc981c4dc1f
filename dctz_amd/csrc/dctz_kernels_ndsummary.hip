// dctz_kernels_ndsummary.hip -- per-tile summaries of an array compressed in 8 x 8 / 4 x 4 x 4 tiles, and of its error
// against the original in place (include/dctz_hip.h: dctzhip_tile_summary_nd).
//
// The record is the flat call's (dctz_kernels_summary.hip), one per stream tile of 64 blocks, over the tile's REAL positions:
// position q = 64 B + j, block B row-major over the block grid, j row-major inside the brick, is real iff every coordinate
// lies inside the array.  The streams carry repeated samples at the padded positions; none of them enters a field, and the
// original is never read there.
//
// k_ndsummary: one wave per stream tile, lane b = block b, grid-stride over the tiles.  (Not named k_tile_summary_...: the flat
// family's budget test counts every kernel of that prefix.)
//   REF = false   summary_tile_values_nd (dctz_summary_head.h) stops with the lane's block in registers, so the tile needs no
//                 image: 16 KiB of staged coefficients, two waves per SIMD.  Whether place j is real is separable per axis
//                 (j_a < d_a - e B_a), so the lane reduces its 64 registers under a 64-bit mask built once per tile.
//                 Order: lane b takes the places j = 0 .. 63 of block b into four running sums over j mod 4.
//   REF = true    k_ndfix_mark's route: ra_tile_image leaves the tile in LDS (NdImage), and the tile is walked in the row
//                 strips k_decompress_ndbox stores, so that the original is read in place in whole row pieces, loaded in
//                 batches of half a tile behind the decode, under the real-position predicate.  Where mark takes ballots, the
//                 lane reduces its strip elements.
//                 Order: lane l takes, for step s = 0 .. e - 1 and in-block row r = 0 .. 64 / e - 1, in-row offset l mod e of
//                 block l / e + (64 / e) s of the tile, into two running sums over r mod 2.
// The running sums join as (0 + 1) + (2 + 3) / as 0 + 1, the lanes in a butterfly (partners 32, 16, .. 1 apart); a position
// that is not real adds nothing.  The order depends on the geometry alone.  Lanes 0-7 store the record as one 64-byte row.
// Every r comes out of the decoders' own functions in their order -- the index check, dequantise_positional,
// block_inv<GEOM>, the de-scale multiply -- and is bit for bit the element dctzhip_decompress_nd writes.
#include "dctz_nd_image.h"
#include "dctz_summary_head.h"

namespace dctz {

// One element into the running values when `ok`: r = v, and with REF the original o beside it
template <typename T, bool REF>
__device__ __forceinline__ void nd_summary_take(SumRec& a, double& s, double& q, double& eq, const bool ok, const T v, const T o) {
  const double d = (double)v;
  a.v[0] = ok ? fmin(a.v[0], d) : a.v[0];
  a.v[1] = ok ? fmax(a.v[1], d) : a.v[1];
  s = ok ? s + d : s;
  q = ok ? q + d * d : q;
  if constexpr (REF) {
    const double dx = (double)o;
    const T er = o - v;                                                // util.c:72-73 / :88-89: difference and square in the data type
    a.v[4] = ok ? fmin(a.v[4], dx) : a.v[4];
    a.v[5] = ok ? fmax(a.v[5], dx) : a.v[5];
    a.v[6] = ok ? fmax(a.v[6], (double)fabs(er)) : a.v[6];
    eq = ok ? eq + (double)(er * er) : eq;
  }
}

template <typename T, int MODE, int GEOM, bool REF>
// (fp32 with the original: the image leaves room for two waves per SIMD, so the registers are held to 256)
__global__ __launch_bounds__(64, (REF && sizeof(T) == 4) ? 2 : 1) void k_ndsummary(NdSummaryParams<T> p) {
  using G = NdImage<T, GEOM>;
  constexpr unsigned E = GEOM == GEOM_2D ? 8u : 4u;                    // block edge
  constexpr int ROWS = 64 / (int)E;                                    // in-block rows of E elements
  constexpr unsigned BPS = 64u / E;                                    // blocks per step
  // steps whose loads of the original are in flight together: half the tile.  (k_ndfix_mark takes an fp32 tile whole; beside
  // the record's running values that is more than the 256 registers two waves per SIMD leave a lane.)
  constexpr unsigned SB = E / 2u;
  constexpr int NS = REF ? 2 : 4;                                      // running sums per field (REF, fp64: four would spill beside a batch of loads)
  __shared__ __attribute__((aligned(16))) unsigned char lds[REF ? G::BYTES : 63 * 64 * 4];
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const unsigned nbx = p.nb[2], nby = p.nb[1];
  const unsigned dx = p.d[2], dy = p.d[1], dz = p.d[0];
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned b1 = min(b0 + (unsigned)TILE_BLKS, p.nfull);
    SumRec a;
    double s[NS], q[NS], eq[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) { s[k] = 0.0; q[k] = 0.0; eq[k] = 0.0; }
    if constexpr (!REF) {
      T x[64];
      if (!summary_tile_values_nd<T, MODE, GEOM>(p, t, lane, tab, qtl, scale, reinterpret_cast<float*>(lds), x)) { bad = true; continue; }
      unsigned long long real = 0ull;                                  // (a lane beyond the last block takes nothing)
      if (b0 + (unsigned)lane < b1) {
        unsigned bz, by, bx;
        ndfix_block<GEOM>(b0 + (unsigned)lane, nbx, nby, bz, by, bx);
        real = nd_real_mask<GEOM>(bz, by, bx, dz, dy, dx);
      }
      a.init();
#pragma unroll
      for (int j = 0; j < 64; j++) nd_summary_take<T, false>(a, s[j & 3], q[j & 3], eq[j & 3], (real >> j) & 1ull, x[j], T(0));
    } else {
      const T* const img = reinterpret_cast<const T*>(lds);
      const T* __restrict__ const ref = p.ref;
      if (!ra_tile_image<T, MODE, GEOM, G>(p, t, lane, tab, qtl, scale, lds)) { bad = true; continue; }
      a.init();
      // k_ndfix_mark's walk: the original's strip elements of SB steps are issued together behind the decode, one round trip per
      // batch; a position that is not real is not loaded and enters nothing
#pragma unroll
      for (unsigned h = 0; h < E; h += SB) {
        asm volatile("" ::: "memory");                                 // (a batch's loads stay behind the decode and behind the batch in front)
        T o[SB][ROWS];
        unsigned long long real = 0ull;                                // bit ROWS i + r: this lane's position of step h + i, row r is real
#pragma unroll
        for (unsigned i = 0; i < SB; i++) {
          const unsigned B = b0 + (unsigned)lane / E + BPS * (h + i);  // block of the tile, in-row offset
          unsigned bz, by, bx;
          ndfix_block<GEOM>(B, nbx, nby, bz, by, bx);                  // once per lane and step
          const unsigned x = bx * E + (unsigned)lane % E;
          const bool in = B < b1 && x < dx;
#pragma unroll
          for (int r = 0; r < ROWS; r++) {
            const unsigned z = GEOM == GEOM_3D ? bz * 4u + (unsigned)(r >> 2) : 0u;
            const unsigned y = GEOM == GEOM_3D ? by * 4u + (unsigned)(r & 3) : by * 8u + (unsigned)r;
            const bool ok = in && z < dz && y < dy;
            o[i][r] = T(0);
            if (ok) o[i][r] = ref[((size_t)z * dy + y) * dx + x];
            real |= (unsigned long long)ok << (i * (unsigned)ROWS + (unsigned)r);
          }
        }
#pragma unroll
        for (unsigned i = 0; i < SB; i++) {
          const T* const src = img + ((unsigned)lane / E + BPS * (h + i)) * (unsigned)G::STRIDE + (unsigned)lane % E;
#pragma unroll
          for (int r = 0; r < ROWS; r++)
            nd_summary_take<T, true>(a, s[r & 1], q[r & 1], eq[r & 1], (real >> (i * (unsigned)ROWS + (unsigned)r)) & 1ull, src[r * (int)E], o[i][r]);
        }
      }
    }
    if constexpr (REF) {
      a.v[2] = s[0] + s[1]; a.v[3] = q[0] + q[1]; a.v[7] = eq[0] + eq[1];
    } else {
      a.v[2] = (s[0] + s[1]) + (s[2] + s[3]);
      a.v[3] = (q[0] + q[1]) + (q[2] + q[3]);
    }
    sum_wave<REF ? 8 : 4>(a);
    if constexpr (!REF) { a.v[4] = 0.0; a.v[5] = 0.0; }                // no original: the four fields are zero
    const double v = sum_field_of_lane(a, lane);
    if (lane < 8) reinterpret_cast<double*>(p.recs + t)[lane] = v;
    if constexpr (REF) __syncthreads();                                // the image is read out before the next tile's staging
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The instantiation of (mode, geometry, with an original)
template <typename T>
auto ndsummary_kernel(int mode, int geom, bool ref) -> void (*)(NdSummaryParams<T>) {
  using Fn = void (*)(NdSummaryParams<T>);
  return with_mode_bool2(mode, geom == GEOM_3D, ref,
                         [](auto M, auto D3, auto R) -> Fn { return k_ndsummary<T, M(), D3() ? GEOM_3D : GEOM_2D, R()>; });
}
template <typename T>
int ndsummary_occupancy(int mode, int geom, bool ref) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)ndsummary_kernel<T>(mode, geom, ref), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_tile_summary_nd(const NdSummaryParams<T>& p, int mode, int geom, bool ref, int grid, hipStream_t s) {
  hipLaunchKernelGGL(ndsummary_kernel<T>(mode, geom, ref), dim3(grid), dim3(64), 0, s, p);
}
template int ndsummary_occupancy<double>(int, int, bool);
template int ndsummary_occupancy<float>(int, int, bool);
template void launch_tile_summary_nd<double>(const NdSummaryParams<double>&, int, int, bool, int, hipStream_t);
template void launch_tile_summary_nd<float>(const NdSummaryParams<float>&, int, int, bool, int, hipStream_t);

}  // namespace dctz
