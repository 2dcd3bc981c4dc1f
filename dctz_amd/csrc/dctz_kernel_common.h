// dctz_kernel_common.h -- device helpers shared by the two kernel files: streaming accesses, the wave scan, the exact
// division by a launch constant (FastDiv), the tile range of a workgroup, the tile image in LDS (TileMap, LDS-DMA issue,
// LDS <-> registers), the statistics accumulator, the QT (de-)normalisation, the mailbox publish, small reductions,
// binning / bin centres, the "stored exactly" flags, the de-quantise step of every decoder, the short last block.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dct64_block.h"
#include "dct_nd_block.h"
#include "dct64_block_pk.h"
#include "dctz_device.h"

namespace dctz {


typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
// The twiddle block is written once at context creation and never by a kernel: reading it through the constant
// address space lets the compiler use scalar loads (the table indices are compile-time constants, the base is a
// kernel argument: wave-uniform).  A plain global pointer gets VECTOR loads here, because the kernels also store to
// global memory and nothing tells the compiler that the table is not among the targets.
template <typename T> using CTab = const __attribute__((address_space(4))) T*;
template <typename T> __device__ __forceinline__ CTab<T> as_ctab(const T* p) { return (CTab<T>)(p); }
// LDS-DMA: 16 bytes per lane, HBM -> LDS (lane l lands at lds + 16 l), through a buffer descriptor (range-checked: zeros
// beyond the end).  Device pass only (the host pass of hipcc does not know the builtin).
#if defined(__HIP_DEVICE_COMPILE__)
#define DMA16(rsrc, lds, voff, soff, aux) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, LDS_PTR(lds), 16, voff, soff, 0, aux)
#else
#define DMA16(rsrc, lds, voff, soff, aux) ((void)0)
#endif

// LDS stores the compiler does not see as such.  A pending LDS-DMA (the next tile on its way into its image) makes the
// compiler put `s_waitcnt vmcnt(0)` in front of every LDS STORE it cannot prove disjoint from the DMA's target -- and
// it proves that for loads only (the disassembly of round 2's k_compress had such a wait in front of every parked
// group: the DMA that was meant to land under the arithmetic was waited for at the first store behind its issue).  The
// staging buffers these helpers write are arrays of their own, never a DMA target.  LDS operations of a wave execute
// in order, so a compiler-visible load behind such a store sees its data.
__device__ __forceinline__ unsigned lds_offset(const void* p) { return (unsigned)(size_t)LDS_PTR(p); }
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void lds_store_b8(unsigned at, unsigned v) { asm volatile("ds_write_b8 %0, %1" :: "v"(at), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_store_b32(unsigned at, unsigned v) { asm volatile("ds_write_b32 %0, %1" :: "v"(at), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_store_b64(unsigned at, u32x2 v) { asm volatile("ds_write_b64 %0, %1" :: "v"(at), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_store_b128(unsigned at, u32x4 v) { asm volatile("ds_write_b128 %0, %1" :: "v"(at), "v"(v) : "memory"); }
#else
__device__ __forceinline__ void lds_store_b8(unsigned, unsigned) {}
__device__ __forceinline__ void lds_store_b32(unsigned, unsigned) {}
__device__ __forceinline__ void lds_store_b64(unsigned, u32x2) {}
__device__ __forceinline__ void lds_store_b128(unsigned, u32x4) {}
#endif
// (the same for LDS atomics without a return value: a store as far as the wait insertion is concerned)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void lds_max_u32(unsigned at, unsigned v) { asm volatile("ds_max_u32 %0, %1" :: "v"(at), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_max_u64(unsigned at, unsigned long long v) { asm volatile("ds_max_u64 %0, %1" :: "v"(at), "v"(v) : "memory"); }
#else
__device__ __forceinline__ void lds_max_u32(unsigned, unsigned) {}
__device__ __forceinline__ void lds_max_u64(unsigned, unsigned long long) {}
#endif
__device__ __forceinline__ void lds_max_bits(unsigned at, unsigned v) { lds_max_u32(at, v); }
__device__ __forceinline__ void lds_max_bits(unsigned at, unsigned long long v) { lds_max_u64(at, v); }
__device__ __forceinline__ void lds_store_item(unsigned at, float v) { lds_store_b32(at, __builtin_bit_cast(unsigned, v)); }
__device__ __forceinline__ void lds_store_item(unsigned at, double v) { lds_store_b64(at, __builtin_bit_cast(u32x2, v)); }

// ------------------------------------------------------------------ helpers --
// Streaming (read-once / write-once) 16-byte accesses: the `nt` policy.  A pure 1 GiB read stream
// runs at 6.8-7.1 TB/s with nt loads against 6.0-6.3 TB/s with plain ones (tools/ubench/stream_read.hip).
template <typename V>
__device__ __forceinline__ V load_stream(const V* p) {
  static_assert(sizeof(V) == 16, "16-byte vectors only");
  const u32x4 r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  V v;
  __builtin_memcpy(&v, &r, 16);
  return v;
}
template <typename V>
__device__ __forceinline__ void store_stream(V* p, const V& v) {
  static_assert(sizeof(V) == 16, "16-byte vectors only");
  u32x4 r;
  __builtin_memcpy(&r, &v, 16);
  __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(p));
}

// Inclusive prefix sum over the 64 lanes of a wavefront with DPP row shifts / row broadcasts
// (six dependent VALU steps instead of six ds_bpermute round trips through the LDS pipe).
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);    // row_shr:1
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);    // row_shr:2
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);    // row_shr:4
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);    // row_shr:8
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
  v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
  return v;
}

__device__ __forceinline__ unsigned long long to_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned int to_bits(float v) { return __float_as_uint(v); }

// ----------------------------------------------- division by a kernel constant --
// x / d with d uniform over the launch (the scaling factor, the bin width).
// hipcc expands an IEEE division into: v_div_scale x2, v_rcp, two (f64) / one (f32)
// Newton steps on the reciprocal, q = x*y, r = fma(-d, q, x), fma(r, y, q) [f32:
// one more residual step], v_div_fmas, v_div_fixup.  Everything up to the
// reciprocal y depends on d alone, and the scale/fixup steps are the identity
// while the exponents of x, d and x/d stay away from the overflow / denormal
// ends.  So: y is computed once per thread with the very same instructions, x is
// checked against a conservative exponent window, and inside it the remaining
// 3 (f64) / 5 (f32) operations give bit-for-bit what `x / d` gives.  Outside the
// window (and for zeros, whose sign v_div_fixup restores) the full division runs.
// tests/test_gpu_parity.py::test_fast_division_is_exact checks the identity on
// the GPU against the compiler's own division.
template <typename T> struct FastDiv;
template <> struct FastDiv<double> {
  double d, y;
  bool ok;                       // host: |d| in [2^-250, 2^250]
  __device__ __forceinline__ void init(double dd, bool okk) {
    d = dd; ok = okk;
    double r = __builtin_amdgcn_rcp(dd);
    double e = fma(-dd, r, 1.0); r = fma(r, e, r);
    e = fma(-dd, r, 1.0); r = fma(r, e, r);
    // the divisor is a kernel argument, so y is wave-uniform: keep it in SGPRs
    y = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(r)),
                         __builtin_amdgcn_readfirstlane(__double2loint(r)));
  }
  __device__ __forceinline__ double core(double x) const {
    const double q = x * y;
    const double r = fma(-d, q, x);
    return fma(r, y, q);
  }
  __device__ __forceinline__ double div(double x) const {          // any x
    const unsigned ex = ((unsigned)__double2hiint(x) >> 20) & 0x7ffu;
    if (ok && (ex - 523u) <= 1000u) return core(x);                // |x| in [2^-500, 2^501)
    if (ok && x == 0.0) return x * y;                              // signed zero
    return x / d;
  }
};
template <> struct FastDiv<float> {
  float d, y;
  bool ok;                       // host: |d| in [2^-30, 2^30]
  __device__ __forceinline__ void init(float dd, bool okk) {
    d = dd; ok = okk;
    const float r = __builtin_amdgcn_rcpf(dd);
    const float e = fmaf(-dd, r, 1.0f);
    y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fmaf(e, r, r))));   // wave-uniform -> SGPR
  }
  __device__ __forceinline__ float core(float x) const {
    const float q = x * y;
    const float r = fmaf(-d, q, x);
    const float q2 = fmaf(r, y, q);
    const float r2 = fmaf(-d, q2, x);
    return fmaf(r2, y, q2);
  }
  // two quotients at once with the packed fp32 instructions of gfx950 (v_pk_mul_f32 / v_pk_fma_f32: the same IEEE
  // operations per component, half the issue slots)
  __device__ __forceinline__ f32x2 core2(f32x2 x) const {
    const f32x2 dd = {d, d}, yy = {y, y};
    const f32x2 q = x * yy;
    const f32x2 r = __builtin_elementwise_fma(-dd, q, x);
    const f32x2 q2 = __builtin_elementwise_fma(r, yy, q);
    const f32x2 r2 = __builtin_elementwise_fma(-dd, q2, x);
    return __builtin_elementwise_fma(r2, yy, q2);
  }
  __device__ __forceinline__ float div(float x) const {
    const unsigned ex = (__float_as_uint(x) >> 23) & 0xffu;
    if (ok && (ex - 64u) <= 126u) return core(x);                  // |x| in [2^-63, 2^64)
    if (ok && x == 0.0f) return x * y;
    return x / d;
  }
};

// (call sites shared by the fp64 instantiations, where the packed form does not exist and the branch is compiled out)
__device__ __forceinline__ f32x2 fastdiv_core2(const FastDiv<float>& d, f32x2 x) { return d.core2(x); }
__device__ __forceinline__ f32x2 fastdiv_core2(const FastDiv<double>&, f32x2 x) { return x; }

// Workgroup b of G owns the contiguous tiles [lo, hi) -- the same partition in k_compress / k_compact_ac
// and in k_decompress.
struct TileRange { unsigned lo, hi; };
__host__ __device__ __forceinline__ TileRange tile_range(unsigned b, unsigned G, unsigned ntiles) {
  const unsigned q = ntiles / G, r = ntiles % G;
  TileRange tr;
  tr.lo = b * q + (b < r ? b : r);
  tr.hi = tr.lo + q + (b < r ? 1u : 0u);
  return tr;
}

// ---------------------------------------------------------- the tile in LDS --
// A tile's image in LDS is made of 1 KiB ROWS; row (jg, s) holds segment s (128 bytes) of the 8 blocks
// 8 jg .. 8 jg + 7, and inside a block's 128 bytes the 16-byte chunks are XOR-swizzled with f(block).  A row is what ONE
// LDS-DMA instruction writes (lane l -> bytes [16 l, 16 l + 16) of the row) and what one 16-byte-per-lane store
// instruction reads back, and lane l's share of a row is a piece of a whole 128-byte line in HBM.  Lane b = block b
// moves chunk ch of its block with ds_read_b128 / ds_write_b128 at lds_a[ch & 7] + (ch >> 3) * 1024.
// The two directions bank differently on gfx950 (MI355X guide, LDS table):
//   * ds_read_b128: groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... ; bank = (a / 4) mod 64.  Lane b's
//     address mod 256 is (b & 1) * 128 + (g ^ f) * 16, so f has to differ between the lanes of equal parity of a group;
//   * ds_write_b128: groups of 8 CONTIGUOUS lanes; bank = (a / 4) mod 32, i.e. only (g ^ f) * 16 counts: f has to take
//     8 different values over b & 7.
// f = (b & 7) ^ ((b >> 4) & 1) does both.  Rounds 1-3 used f = (b >> 1) & 7 (DCTZ_SWZ = 0), which is right for the reads
// and 2-way conflicted for every write of the image: k_decompress's 32 writes per tile made 9.07 M of its 22.05 M
// LDS-array cycles conflict cycles (41 %, profiles/r03_pmc.txt).
#ifndef DCTZ_SWZ
#define DCTZ_SWZ 1
#endif
template <typename T, int PH>
struct TileMap {
  using G = Geo<T, PH>;
  int lds_a[8];        // LDS byte offset of chunk class g = ch & 7 of this lane's block (row part of segment 0)
  int g_even, g_odd;   // HBM byte offset (inside a tile) of this lane's 16 bytes of row (jg, 0), for odd_row(jg) false / true
  // which of the two a row takes: the part of f that comes from the row's number
  static __host__ __device__ constexpr bool odd_row(int jg) { return DCTZ_SWZ ? (jg & 2) != 0 : (jg & 1) != 0; }
  __device__ __forceinline__ int g_of(int jg) const { return odd_row(jg) ? g_odd : g_even; }
  __device__ __forceinline__ void init(int lane) {
    const int f = DCTZ_SWZ ? ((lane & 7) ^ ((lane >> 4) & 1)) : ((lane >> 1) & 7);
#pragma unroll
    for (int g = 0; g < 8; g++) lds_a[g] = (lane >> 3) * G::SEGP * 1024 + (lane & 7) * 128 + ((g ^ f) * 16);
    // as lane l of a ROW instruction: slot l of the row = chunk class (l & 7) ^ f(block) of block 8 jg + (l >> 3)
    const int beta = lane >> 3, gam = lane & 7;
    g_even = beta * G::BLKB + ((gam ^ (DCTZ_SWZ ? beta : (beta >> 1))) * 16);
    g_odd = g_even ^ (DCTZ_SWZ ? 16 : 64);
  }
};
// (the same for the multi-dimensional forms, which compute their chunk per row: chunk class of row-instruction lane
// (beta, gam) in row jg)
__device__ __forceinline__ int swz_row_chunk(int beta, int gam, int jg) {
  return DCTZ_SWZ ? (gam ^ beta ^ ((jg >> 1) & 1)) : (gam ^ (beta >> 1) ^ ((jg & 1) << 2));
}

// HBM -> LDS, one phase of a tile, no registers.  rsrc covers the workgroup's input range; the range check
// zero-fills whatever lies beyond the last whole block.
// (JG0, JG1: the rows of block groups [JG0, JG1) only -- k_compress issues a phase in pieces, between its other work)
template <typename T, int PH, int JG0 = 0, int JG1 = 8>
__device__ __forceinline__ void issue_phase_dma(__amdgpu_buffer_rsrc_t rsrc, unsigned rel, int phase, unsigned char* tilebuf, const TileMap<T, PH>& tm) {
  using G = Geo<T, PH>;
  const int base = (int)(rel * (unsigned)G::TILEB) + phase * G::SEGP * 128;
#pragma unroll
  for (int jg = JG0; jg < JG1; jg++)
#pragma unroll
    for (int s = 0; s < G::SEGP; s++)
      DMA16(rsrc, tilebuf + (jg * G::SEGP + s) * 1024, tm.g_of(jg), base + jg * 8 * G::BLKB + s * 128, 2 /* nt */);
}

// ---- multi-dimensional blocks straight from / to the array (NdDirect) ----
// Byte offset of the origin of block B of the tile grid, or an offset beyond any descriptor range for B >= nblk
// (loads return zeros there, stores are dropped).
template <typename T>
__device__ __forceinline__ unsigned nd_block_origin(const NdDirect& nd, unsigned B) {
  auto divmod = [](unsigned a, unsigned d, unsigned m, unsigned& r) {
    unsigned q = __umulhi(a, m);                     // m = floor(2^32 / d): q is the quotient or one short of it
    r = a - q * d;
    if (r >= d) { q++; r -= d; }
    return q;
  };
  unsigned bx, elem;
  const unsigned t = divmod(B, nd.nbx, nd.mx, bx);
  if (nd.nd == 2) {
    elem = t * 8u * nd.dx + bx * 8u;
  } else {
    unsigned by;
    const unsigned bz = divmod(t, nd.nby, nd.my, by);
    elem = (bz * 4u * nd.dy + by * 4u) * nd.dx + bx * 4u;
  }
  return B < nd.nblk ? elem * (unsigned)sizeof(T) : 0xFFFFFFF0u;
}
// Byte offset, inside its block's footprint in the array, of 16-byte chunk ch of the block (chunk ch = elements
// [ch * EPV, ch * EPV + EPV) of the row-major tile: always inside one row of the tile)
template <typename T>
__device__ __forceinline__ unsigned nd_chunk_offset(const NdDirect& nd, int ch) {
  const unsigned j0 = (unsigned)ch * (unsigned)Traits<T>::EPV;
  if (nd.nd == 2) return ((j0 >> 3) * nd.dx + (j0 & 7u)) * (unsigned)sizeof(T);
  return (((j0 >> 4) * nd.dy + ((j0 >> 2) & 3u)) * nd.dx + (j0 & 3u)) * (unsigned)sizeof(T);
}
// HBM -> LDS, one phase of a tile of a multi-dimensional array: same image in LDS as issue_phase_dma builds for the
// flat layout (row (jg, s) = segment s of blocks 8 jg .. 8 jg + 7, chunks XOR-swizzled), other addresses in HBM.
template <typename T, int PH>
__device__ __forceinline__ void issue_phase_dma_nd(__amdgpu_buffer_rsrc_t rsrc, const NdDirect& nd, unsigned tile, int phase, unsigned char* tilebuf, int lane) {
  using G = Geo<T, PH>;
  const int beta = lane >> 3, gam = lane & 7;
#pragma unroll
  for (int jg = 0; jg < 8; jg++) {
    const unsigned org = nd_block_origin<T>(nd, tile * (unsigned)TILE_BLKS + (unsigned)(8 * jg + beta));
    const int cg = swz_row_chunk(beta, gam, jg);                       // chunk of the segment this lane moves (TileMap's swizzle)
#pragma unroll
    for (int s = 0; s < G::SEGP; s++) {
      const unsigned off = org + nd_chunk_offset<T>(nd, 8 * (phase * G::SEGP + s) + cg);
      DMA16(rsrc, tilebuf + (jg * G::SEGP + s) * 1024, (int)(org >= 0xFFFFFFF0u ? org : off), 0, 2 /* nt */);
    }
  }
}

// LDS image of phase PHASE -> this lane's elements [PHASE * 64 / PH, (PHASE + 1) * 64 / PH) of its block
template <typename T, int PH, int PHASE>
__device__ __forceinline__ void read_phase(T (&x)[64], const unsigned char* tilebuf, const TileMap<T, PH>& tm) {
  using Vec = typename Traits<T>::Vec;
  using G = Geo<T, PH>;
  constexpr int EPV = Traits<T>::EPV;
#pragma unroll
  for (int ch = 0; ch < G::CHP; ch++) {
    const Vec v = *reinterpret_cast<const Vec*>(tilebuf + tm.lds_a[ch & 7] + (ch >> 3) * 1024);
    Traits<T>::unpack(v, &x[(PHASE * G::CHP + ch) * EPV]);
  }
}

template <typename T, int PH, int PHASE>
__device__ __forceinline__ void write_phase(const T (&x)[64], unsigned char* tilebuf, const TileMap<T, PH>& tm) {
  using Vec = typename Traits<T>::Vec;
  using G = Geo<T, PH>;
  constexpr int EPV = Traits<T>::EPV;
#pragma unroll
  for (int ch = 0; ch < G::CHP; ch++)
    *reinterpret_cast<Vec*>(tilebuf + tm.lds_a[ch & 7] + (ch >> 3) * 1024) = Traits<T>::pack(&x[(PHASE * G::CHP + ch) * EPV]);
}

// ---------------------------------------------------- statistics on the fly --
// calc_data_stat's reductions (util.c:18-25 / :31-38).
template <typename T>
struct StatAcc {
  T mx, mn;
  double sum;                                      // raw-domain sum (or correction term)
  double dcs;                                      // fused path: sum of the blocks' DC coefficients (see k_compress)
  __device__ __forceinline__ void init() { mx = T(0); mn = Traits<T>::huge(); sum = 0.0; dcs = 0.0; }
  // A NaN element is passed over, like `a > mx ? a : mx`.  Kernels run in IEEE mode, where v_max /
  // v_min skip a QUIET NaN operand but answer a SIGNALLING one with a quiet NaN -- which the next element then replaces:
  // the lane has lost its maximum so far (seen on an MI355X: sf a decade or two short when signalling NaNs followed the
  // array's largest value in its block).  So |x| is canonicalised first -- v_max(|x|, |x|) quiets a signalling NaN and
  // leaves everything else as it is -- and the running values meet quiet NaNs only: three instructions per element for
  // what were two.
  __device__ __forceinline__ void add(T e, bool in_sum) {
    minmax(e);
    if (in_sum) sum += (double)e;
  }
  __device__ __forceinline__ void minmax(T e) {
    T a;
    if constexpr (sizeof(T) == 8) {
      asm("v_max_f64 %0, |%1|, |%1|" : "=v"(a) : "v"(e));
      asm("v_max_f64 %0, %1, %2" : "=v"(mx) : "v"(mx), "v"(a));
      asm("v_min_f64 %0, %1, %2" : "=v"(mn) : "v"(mn), "v"(a));
    } else {
      asm("v_max_f32 %0, |%1|, |%1|" : "=v"(a) : "v"(e));
      asm("v_max_f32 %0, %1, %2" : "=v"(mx) : "v"(mx), "v"(a));
      asm("v_min_f32 %0, %1, %2" : "=v"(mn) : "v"(mn), "v"(a));
    }
  }
  // workgroup reduction -> part[3*slot .. 3*slot+2]; `s` is scratch for 3 * (threads/64) doubles
  // dc_scale: raw-domain value of one unit of DC (8 * sf for 64-element orthonormal blocks)
  __device__ __forceinline__ void flush(double* part, unsigned slot, double* s, int nwaves, double dc_scale = 0.0) {
    double dmx = (double)mx, dmn = (double)mn, sm = sum + dcs * dc_scale;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      dmx = fmax(dmx, __shfl_down(dmx, d));
      dmn = fmin(dmn, __shfl_down(dmn, d));
      sm += __shfl_down(sm, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s[wave] = dmx; s[nwaves + wave] = dmn; s[2 * nwaves + wave] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < nwaves; w++) { dmx = fmax(dmx, s[w]); dmn = fmin(dmn, s[nwaves + w]); sm += s[2 * nwaves + w]; }
      part[3 * slot + 0] = dmx;
      part[3 * slot + 1] = dmn;
      part[3 * slot + 2] = sm;
    }
  }
};

// QT normalisation of an out-of-range coefficient (dctz-comp-lib.c:488-492 /
// :514-518); error_bound is a double there, so f32 evaluates product and sum in
// double and rounds once.
__device__ __forceinline__ double qt_normalise(double item, double q, double eb, double qf, double rmin, double rmax) {
  if (item < rmin) return (item / q) * eb * qf + rmin;
  if (item > rmax) return (item / q) * eb * qf + rmax;
  return item;
}
__device__ __forceinline__ float qt_normalise(float item, float q, double eb, float qf, float rmin, float rmax) {
  if (item < rmin) return (float)((double)(item / q) * eb * (double)qf + (double)rmin);
  if (item > rmax) return (float)((double)(item / q) * eb * (double)qf + (double)rmax);
  return item;
}
// QT de-normalisation on decode (dctz-decomp-lib.c:404-409 / :450-454)
__device__ __forceinline__ double qt_restore(double v, double q, double eb, double qf, double rmin, double rmax) {
  return (v > 0) ? ((v - rmax) / (eb * qf)) * q : ((v - rmin) / (eb * qf)) * q;
}
__device__ __forceinline__ float qt_restore(float v, float q, double eb, float qf, float rmin, float rmax) {
  return (v > 0) ? (float)(((double)(v - rmax) / (eb * (double)qf)) * (double)q)
                 : (float)(((double)(v - rmin) / (eb * (double)qf)) * (double)q);
}

// The QT table on decode: lane j of a register (pair) holds qtable[j]; entry j -- j a compile-time constant at every use --
// comes out with v_readlane into scalar registers.  (Rounds 2-3 kept the table in LDS: every flagged position of a tile
// then was an LDS round trip inside its branch, with one wave per SIMD nothing to hide it behind -- the QT decoder waited
// 76 % longer than its EC twin for 4 % FEWER vector instructions, profiles/r04_pmc_qt.txt.)
template <typename T> struct QtLanes;
template <> struct QtLanes<double> {
  int lo, hi;
  __device__ __forceinline__ void load(const double* qtab, int lane) { const double v = qtab[lane]; lo = __double2loint(v); hi = __double2hiint(v); }
  __device__ __forceinline__ double at(int j) const { return __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j)); }
};
template <> struct QtLanes<float> {
  int w;
  __device__ __forceinline__ void load(const float* qtab, int lane) { w = __float_as_int(qtab[lane]); }
  __device__ __forceinline__ float at(int j) const { return __int_as_float(__builtin_amdgcn_readlane(w, j)); }
};

// ------------------------------------------------------------- host hand-off --
// System-scope release of a sequence number into the HostBox (fine-grained pinned host
// memory): everything this thread (and, after a barrier, its workgroup) wrote to the
// box before is visible to the polling host thread once it reads the number.
__device__ __forceinline__ void box_publish(volatile unsigned long long* flag, unsigned long long seq) {
  __threadfence_system();
  __hip_atomic_store(const_cast<unsigned long long*>(flag), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// reduction of {max, min, sum} partials by one workgroup (any size up to 256 threads); thread 0 returns with the result
__device__ __forceinline__ void reduce_parts(const double* __restrict__ part, int nparts, double& dmx, double& dmn, double& sum) {
  dmx = 0.0; dmn = 1.79769313486231570815e308; sum = 0.0;
  for (int i0 = threadIdx.x; i0 < nparts; i0 += 4 * (int)blockDim.x) {      // four entries in flight per thread
    double a[4], b[4], c[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * (int)blockDim.x;
      const bool in = i < nparts;
      a[u] = in ? part[3 * i] : 0.0; b[u] = in ? part[3 * i + 1] : 1.79769313486231570815e308; c[u] = in ? part[3 * i + 2] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { dmx = fmax(dmx, a[u]); dmn = fmin(dmn, b[u]); sum += c[u]; }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    dmx = fmax(dmx, __shfl_down(dmx, d));
    dmn = fmin(dmn, __shfl_down(dmn, d));
    sum += __shfl_down(sum, d);
  }
  __shared__ double s[3][SWG / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  if (lane == 0) { s[0][wave] = dmx; s[1][wave] = dmn; s[2][wave] = sum; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < nw; w++) { dmx = fmax(dmx, s[0][w]); dmn = fmin(dmn, s[1][w]); sum += s[2][w]; }
}

// Sum over a workgroup of one unsigned per thread (every thread gets the total); `sh`: one word per wave
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* sh) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  __syncthreads();                                   // sh[] of an earlier call is consumed
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  unsigned tot = 0;
  for (int w = 0; w < nw; w++) tot += sh[w];
  return tot;
}

// ------------------------------------------------- binning / bin centres --
// Binning of one coefficient (:363-414; conv_tbl :27-43) in floating point:
//   q = (item - range_min) / bin_width  (the reference's own expression, exact division),  f = floor(q)
//   (== the (t_bin_id) truncation for q >= 0),  conv_tbl[f] = |254.5 - 2 f| - 0.5  for f = 0..254, and
//   >= 255 for f >= 255 or f <= -1, which v_cvt_pk_u8_f32 saturates to 255 = "stored exactly" while it
//   packs the byte.  SAFE = false relies on  item > range_max  =>  q >= 255, which the host verifies
//   for the launch constants ((2 range_max) / bin_width >= 255 in T arithmetic); otherwise the
//   reference's range test is applied explicitly (one compare + one select more per coefficient).
template <typename T, bool SAFE>
__device__ __forceinline__ float bin_value(T item, T q, T range_max) {
  const T f = floor(q);
  const T g = fma_(T(-2), f, T(254.5));
  float h = (float)(fabs(g) - T(0.5));
  if (SAFE) h = (fabs(item) > range_max) ? 255.0f : h;       // == (item < range_min || item > range_max): range_min = -range_max
  return h;
}


// bin_center[b] of gen_bins / gen_bins_f (binning.c:17-23 / :37-43) = (T)(b odd ? b/2 + 1 : -(b/2)) * bin_width, computed
// instead of looked up, in the fp64 kernel (a table in LDS is 63 reads per block with bank conflicts wherever the bin ids
// of a position spread over the 64 blocks of a tile: 36 % of the kernel's LDS cycles, profiles/r02_pmc.txt, r03_pmc.txt).  `w1` holds the four
// magnitudes (b + 1) >> 1 of a dword of bin ids as bytes, `nw` the dword's complement (bit 0 of a byte set <=> b even
// <=> the centre is negative).  The magnitude goes byte -> float in one instruction, the sign is or-ed in, and the
// product passes through "+ (+0)": -0 * bin_width + 0 = +0, the table's value for b = 0.
template <typename T>
__device__ __forceinline__ T bin_centre(const unsigned w1, const unsigned nw, const int i, const T bin_width) {
  const float mag = (float)((w1 >> (8 * i)) & 255u);
  const unsigned sgn = (nw << (31 - 8 * i)) & 0x80000000u;
  const float t = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, mag) | sgn);
  if constexpr (sizeof(T) == 8) return __builtin_fma((double)t, bin_width, 0.0);
  else return __builtin_fmaf(t, bin_width, 0.0f);
}
// gen_bins' own expression, for the table and for the short block
template <typename T>
__device__ __forceinline__ T bin_centre_ref(const unsigned b, const T bin_width) {
  const int ti = (b & 1u) ? (int)(b >> 1) + 1 : -(int)(b >> 1);
  return (T)ti * bin_width;
}
// Where a decoder takes the centre of byte i of a dword of bin ids from: computed (bin_centre), or looked up in a table
// in LDS that the workgroup fills first (fp32 of the whole-array decoders: computing measured 6 % slower there).
// (BinDword: what bin_centre needs of a dword, made once per dword -- made per position, the compiler does not merge the
// four and k_decompress_il<double, EC> grows by 140 instructions)
struct BinDword { unsigned w, w1, nw; };                               // four bin ids, their magnitudes (b + 1) >> 1, their complement
__device__ __forceinline__ BinDword bin_dword(const unsigned w) { return {w, ((w >> 1) & 0x7F7F7F7Fu) + (w & 0x01010101u), ~w}; }
template <typename T, bool ARITH> struct BinCentres {
  T bin_width;
  const T* tab;                                                        // !ARITH: 256 entries, fill_bin_centres
  __device__ __forceinline__ T at(const BinDword& d, const int i) const {                        // :416 / :462
    if constexpr (ARITH) return bin_centre<T>(d.w1, d.nw, i, bin_width);
    else return tab[(d.w >> (8 * i)) & 255u];
  }
};
template <typename T>
__device__ __forceinline__ void fill_bin_centres(T* tab, const T bin_width, const int tid, const int nthreads) {
  for (int b = tid; b < 256; b += nthreads) tab[b] = bin_centre_ref<T>((unsigned)b, bin_width);
}

// --------------------------------------------- "stored exactly" flags, de-quantise --
// Bit 7 of byte i set <=> byte i of w, a dword of four bin ids, is 255: the coefficient is stored exactly (:400 / :446)
__device__ __forceinline__ unsigned exact_flags(const unsigned w) {
  const unsigned v = ~w;                                               // a zero byte of v <=> bin id 255
  const unsigned z = ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v;            // bit 7 of a byte set <=> that byte of v is non-zero
  return ~z & 0x80808080u;
}
// (dword g of a block's sixteen: j = 0 is the DC slot, never an exact coefficient, :392 / :438)
__device__ __forceinline__ unsigned block_flags(const unsigned (&w)[16], const int g) {
  return g == 0 ? exact_flags(w[0]) & ~0x80u : exact_flags(w[g]);
}
__device__ __forceinline__ unsigned block_flag_count(const unsigned (&w)[16]) {
  unsigned n = 0;
#pragma unroll
  for (int g = 0; g < 16; g++) n += (unsigned)__popc(block_flags(w, g));
  return n;
}

// De-quantise one block (dctz-decomp-lib.c:389-417 / :438-463): the sixteen dwords of bin ids `w`, the block's DC and the
// tile's piece of AC_exact staged in LDS (`stage`, this lane's first coefficient at `ptr`, reads clamped to `stage_last`)
// -> x[64].  `qtab(j)` is the QT table's entry j (QT only; EC callers pass anything).  The callers keep loading,
// staging, waits, prefetch and stores.  Two forms, because two measured:
//
// GROUPED (fp64, one wave per SIMD, every LDS round trip exposed).  Four coefficients = one dword of bin ids at a time:
// the (up to four) exact coefficients of the group are fetched together -- their places follow from the flag bits alone
// -- so that a tile pays one LDS round trip per GROUP that has a flag somewhere in the wave (16 at most), not one per
// flagged POSITION (63 on noisy data: at p = 17 % the serialised round trips were a third of the kernel; 512^3 fp64:
// 0.33 -> 0.28 ms there, 0.245 -> 0.235 at p = 5 %).
// QT_TRAILING: dctz-decomp-lib.c:404-409 in a pass of its own over the flagged positions.  Inside the loop every division
// sits right behind the LDS read of its coefficient, one exposed round trip per flagged group (with one wave per SIMD the
// QT decoder spent 76 % more cycles waiting than its EC twin for FEWER vector instructions, profiles/r04_pmc_qt.txt);
// behind it the coefficients are in registers already and the reads of all sixteen groups overlap as they do in EC mode.
template <typename T, int MODE, bool QT_TRAILING, typename Centre, typename QTab>
__device__ __forceinline__ void dequantise_grouped(T (&x)[64], const unsigned (&w)[16], const float dc, unsigned& ptr, const float* stage,
                                                   const unsigned stage_last, const Centre centre, QTab&& qtab, const double eb,
                                                   const T range_min, const T range_max) {
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const unsigned m = block_flags(w, g);
    const BinDword d = bin_dword(w[g]);
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (__builtin_amdgcn_ballot_w64(m != 0u)) {                        // :400 / :446 somewhere in the wave
      unsigned at[4];
      at[0] = ptr;
      at[1] = at[0] + ((m >> 7) & 1u);
      at[2] = at[1] + ((m >> 15) & 1u);
      at[3] = at[2] + ((m >> 23) & 1u);
      ptr = at[3] + (m >> 31);
#pragma unroll
      for (int i = 0; i < 4; i++) e[i] = stage[min(at[i], stage_last)];        // (all lanes read: predicating the reads on the flag measured slower)
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = 4 * g + i;
      if (j == 0) { x[0] = (T)dc; continue; }                          // :392 / :438
      T v = centre.at(d, i);
      if ((m >> (8 * i + 7)) & 1u) {
        v = (T)e[i];
        if (MODE == DCTZHIP_QT && !QT_TRAILING) v = qt_restore(v, qtab(j), eb, T(10), range_min, range_max);
      }
      x[j] = v;
    }
  }
  if constexpr (MODE == DCTZHIP_QT && QT_TRAILING) {
#pragma unroll
    for (int g = 0; g < 16; g++) {
      const unsigned m = block_flags(w, g);
      if (__builtin_amdgcn_ballot_w64(m != 0u)) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int j = 4 * g + i;
          if (j != 0 && ((m >> (8 * i + 7)) & 1u)) x[j] = qt_restore(x[j], qtab(j), eb, T(10), range_min, range_max);
        }
      }
    }
  }
}
// POSITIONAL (fp32: several waves per SIMD hide the round trips, the grouped form measured 10 % slower; the range decoder).
// Written as sixteen dwords of four: as ONE loop of 63 trips the compiler leaves it partly rolled in k_decompress_one<float>,
// and the bin ids and the block then live in scratch memory -- 144 bytes per lane, stored and read back per tile: 15 MB of
// the 41 MB that kernel wrote for a 26 MB array (profiles/r05_c2_raw_traffic.txt).
// PIN: each value through a register of its own (same kernel, same file: paired into <2 x float> stores by the vectoriser,
// the first 33 elements of the block stayed an array in scratch memory).
template <typename T, int MODE, bool PIN, typename Centre, typename QTab>
__device__ __forceinline__ void dequantise_positional(T (&x)[64], const unsigned (&w)[16], const float dc, unsigned& ptr, const float* stage,
                                                      const unsigned stage_last, const Centre centre, QTab&& qtab, const double eb,
                                                      const T range_min, const T range_max) {
#pragma unroll
  for (int g = 0; g < 16; g++) {
    const BinDword d = bin_dword(w[g]);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int j = 4 * g + i;
      if (j == 0) { x[0] = (T)dc; continue; }                          // :392 / :438
      T v = centre.at(d, i);
      if (((w[g] >> (8 * i)) & 255u) == 255u) {                        // :400 / :446
        const float e = stage[min(ptr, stage_last)];
        ptr++;
        v = (T)e;
        if (MODE == DCTZHIP_QT) v = qt_restore(v, qtab(j), eb, T(10), range_min, range_max);
      }
      if (PIN) asm volatile("" : "+v"(v));
      x[j] = v;
    }
  }
}

// ------------------------------------------------------- the short last block --
// Length l = N % 64: the reference re-plans a length-l (l even) or 2l (l odd) FFT for it (dctz-comp-lib.c:326-340,
// dct.c:59-72); here a definition-order DFT with host-built roots `rt`, lane k = element / coefficient k, one wave.  The
// phases exchange through LDS: the caller puts its own barrier between them (a workgroup of one wave: __syncthreads;
// one wave of several: its LDS operations are in order, s_waitcnt lgkmcnt(0)) and guards each with k < l.
// Forward: element a -> its mirrored place(s) in v[N]; then coefficient k.
template <typename T>
__device__ __forceinline__ void short_fwd_fill(T* v, const int l, const int k, const T a) {
  if (l & 1) { v[k] = a; v[l + (l - 1 - k)] = a; }                     // dct.c:61-64
  else if (k & 1) v[l - 1 - (k >> 1)] = a;                             // dct.c:75-83
  else v[k >> 1] = a;
}
// (N = short_dft_len(l) comes from the caller, computed in front of its k < l branches as it always was: with N derived in
// here k_compress_one<double, EC> spilled 11 VGPRs for 8)
__device__ __forceinline__ int short_dft_len(const int l) { return (l & 1) ? 2 * l : l; }
template <typename T>
__device__ __forceinline__ T short_fwd_sum(const T* v, const T* rt, const int N, const int k) {
  T sr = T(0), si = T(0);
  for (int j = 0; j < N; j++) {
    const int tt = (j * k) % N;
    sr = sr + v[j] * rt[RTAB_WR + tt];
    si = si + v[j] * rt[RTAB_WI + tt];
  }
  return rt[RTAB_AS + k] * sr + rt[RTAB_AX + k] * si;                  // dct.c:100-102 (Im V = -si)
}
// pass-1 binning of its coefficients, the reference's own form (:363-414)
template <typename T>
__device__ __forceinline__ unsigned bin_short(const T coef, const T range_min, const T range_max, const FastDiv<T>& bwd) {
  const bool out = fabs(coef) > range_max;                             // == (item < range_min || item > range_max)
  const T u = coef - range_min;
  const T q = bwd.ok ? bwd.core(u) : u / bwd.d;
  const int t = (int)q;                                                // (t_bin_id) cast: truncation
  unsigned b = out ? 255u : (unsigned)(t <= 127 ? 254 - 2 * t : 2 * t - 255);   // conv_tbl :27-43 (t == 255 -> 255)
  if (coef != coef) b = 0u;                                            // a NaN coefficient: bin id 0, like bin_value()
  return b;
}
// Inverse (dctz-decomp-lib.c:423-428, dct.c:144-199): coefficient k from its bin id b, the DC, or -- `exc` -- the exact
// value the caller fetched; then a[] -> cr[] / ci[] (128 entries each, cleared first: a barrier between the two as well);
// then element k.
template <typename T, int MODE, typename QTab>
__device__ __forceinline__ T short_inv_value(const unsigned b, const bool exc, const int k, const float dc, T exact, const T bin_width,
                                             QTab&& qtab, const double eb, const T range_min, const T range_max) {
  if (k == 0) return (T)dc;
  if (!exc) return bin_centre_ref<T>(b, bin_width);
  if (MODE == DCTZHIP_QT) exact = qt_restore(exact, qtab(k), eb, T(10), range_min, range_max);
  return exact;
}
template <typename T>
__device__ __forceinline__ void short_inv_clear(T* cr, T* ci, const int k) { cr[k] = T(0); ci[k] = T(0); cr[k + 64] = T(0); ci[k + 64] = T(0); }
template <typename T>
__device__ __forceinline__ void short_inv_spread(T* cr, T* ci, const T* a, const T* rt, const int l, const int k) {
  cr[k] = rt[RTAB_IAS + k] * a[k];                                     // dct.c:146-151 / :166-172
  ci[k] = rt[RTAB_IAX + k] * a[k];
  if ((l & 1) && k >= 1) {                                             // dct.c:152-153
    cr[l + k] = rt[RTAB_IAX + k] * a[l - k];
    ci[l + k] = -(rt[RTAB_IAS + k] * a[l - k]);
  }
}
template <typename T>
__device__ __forceinline__ T short_inv_sum(const T* cr, const T* ci, const T* rt, const int l, const int k) {
  const int N = short_dft_len(l);
  const int s = (l & 1) ? k : ((k & 1) ? l - 1 - (k >> 1) : (k >> 1)); // dct.c:189-199
  T acc = T(0);
  for (int j = 0; j < N; j++) {
    const int tt = (s * j) % N;
    acc = acc + (cr[j] * rt[RTAB_WR + tt] - ci[j] * rt[RTAB_WI + tt]);
  }
  return (l & 1) ? (acc / (T)l) / T(2) : acc / (T)l;                   // dct.c:163 / :185
}

// ---- one tile for random access (k_decompress_range, k_decompress_box) ------------------------------------------------------
// LDS image of a reconstructed tile: block b at elements [b * STRIDE, b * STRIDE + 64), one 16-byte pad behind every
// block, so that the lanes' 16-byte writes of their own blocks (rows STRIDE elements apart) and the reads in output order
// (consecutive elements across the lanes) both spread over the banks.  The tile's exact coefficients (up to 63 * 64
// floats) are staged in the same array before the image is written.
template <typename T> struct RaGeo {
  static constexpr int EPV = Traits<T>::EPV;
  static constexpr int STRIDE = 64 + EPV;
  static constexpr int BYTES = TILE_BLKS * STRIDE * (int)sizeof(T);
  static_assert(BYTES >= 63 * 64 * 4, "a dense tile's exact coefficients fit the image");
  // element e of the tile in the image
  __device__ static unsigned at(unsigned e) { return e + (e >> 6) * (unsigned)EPV; }
};

// Tile t of the array into the image, by one wave (lane b = block b): flags and wave scan, the index check, staging of
// AC_exact[idx[t], idx[t + 1]), de-quantisation, inverse transform, de-scaling -- the whole-array decoders' functions in
// their order.  P is RangeParams<T>, BoxParams<T> or NdBoxParams<T>.  False: the index disagrees with the tile's own flags or leaves the
// caller's AC_exact; nothing of AC_exact was read and the image is not written.  True: the image is complete behind the
// closing barrier.  The short last block only contributes its flags (its elements are the _rem kernels').
// GEOM: the block transform (k_decompress_ndbox: the tiles of dctzhip_compress_nd); G: the image, RaGeo's members.
template <typename T, int MODE, int GEOM = GEOM_1D, typename G = RaGeo<T>, typename P>
__device__ __forceinline__ bool ra_tile_image(const P& p, const unsigned t, const int lane, const CTab<T> tab, const QtLanes<T>& qtl,
                                              const bool scale, unsigned char* lds) {
  using Vec = typename Traits<T>::Vec;
  constexpr int EPV = G::EPV;
  float* const stage = reinterpret_cast<float*>(lds);
  T* const img = reinterpret_cast<T*>(lds);
  const unsigned rem = p.n - p.nfull * 64u;
  const unsigned full_end = p.nfull * 64u;
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
  const bool full = blk < p.nfull;
  unsigned w[16];
  float dcv = 0.f;
  unsigned cnt = 0;
  if (full) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    dcv = p.dc[blk];
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0u;
    // the short block's flags count for the tile (its elements are the _rem kernel's: this lane stores nothing)
    if (blk == p.nfull && rem)
      for (unsigned j = 1; j < rem; j++) cnt += p.bin[(size_t)full_end + j] == 255u ? 1u : 0u;
  }
  cnt += block_flag_count(w);
  const unsigned incl = wave_incl_scan(cnt);
  const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
  const unsigned s0 = p.idx[t], s1 = p.idx[t + 1];
  // the index must agree with the tile's own flags and stay inside the caller's AC_exact (else: refused, nothing read)
  if (s1 < s0 || s1 - s0 != tot || s1 > p.ac_count) return false;
  for (unsigned i = (unsigned)lane; i < tot; i += 64u) stage[i] = p.ac[s0 + i];
  __syncthreads();
  unsigned ptr = incl - cnt;                                           // this block's first exact coefficient in the tile
  T x[64];
  dequantise_positional<T, MODE, false>(x, w, dcv, ptr, stage, (unsigned)(63 * 64 - 1), BinCentres<T, true>{p.bin_width, nullptr},
                                        [&](int j) { return qtl.at(j); }, p.eb, p.range_min, p.range_max);
  __syncthreads();                                                     // the staged coefficients are consumed
  block_inv<T, CTab<T>, GEOM, (sizeof(T) == 4)>(x, tab);
  if (scale) {
#pragma unroll
    for (int j = 0; j < 64; j++) x[j] = x[j] * p.sf;                   // dctz-decomp-lib.c:494-511
  }
#pragma unroll
  for (int ch = 0; ch < 64 / EPV; ch++)
    *reinterpret_cast<Vec*>(img + lane * G::STRIDE + ch * EPV) = Traits<T>::pack(&x[ch * EPV]);
  __syncthreads();
  return true;
}

// The short last block (length l = n % 64) of a box that reaches into it, by one wave (k_decompress_box_rem,
// k_decompress_mbox_rem): k_decompress_range_rem with the box test and the box's output position in place of [lo, hi).
// a: 64, cr / ci: 128 elements of LDS.
template <typename T, int MODE, typename P>
__device__ __forceinline__ void box_rem_block(const P& p, const BoxGeo& g, T* const out, const int k, T* a, T* cr, T* ci) {
  const int l = (int)(p.n - p.nfull * 64u);
  const size_t base = (size_t)p.nfull * 64;
  const unsigned t = p.nfull / (unsigned)TILE_BLKS;                    // the tile that holds the short block
  // flags of the tile's whole blocks in front of the short block
  unsigned c = 0;
  const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)k;
  if (blk < p.nfull) {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.bin + (size_t)blk * 64);
    unsigned w[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = src[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    c = block_flag_count(w);
  }
  const unsigned start = p.idx[t] + (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan(c), 63);
  const unsigned lim = min(p.ac_count, p.idx[t + 1]);
  unsigned b = 0;
  if (k < l) b = p.bin[base + k];
  const bool exc = (k < l) && (k != 0) && (b == 255u);
  const unsigned long long msk = __ballot(exc);
  const unsigned rank = (unsigned)__popcll(msk & ((1ull << k) - 1ull));
  short_inv_clear(cr, ci, k);
  if (k < l) {
    T e = T(0);
    if (exc) { if (start + rank < lim) e = (T)p.ac[start + rank]; else atomicExch(&p.ctl->error, 2u); }
    a[k] = short_inv_value<T, MODE>(b, exc, k, k == 0 ? p.dc[p.nfull] : 0.f, e, p.bin_width, [&](int j) { return p.qtab[j]; }, p.eb, p.range_min, p.range_max);
  }
  __syncthreads();
  if (k < l) short_inv_spread(cr, ci, a, p.rtab, l, k);
  __syncthreads();
  if (k < l) {
    T val = short_inv_sum(cr, ci, p.rtab, l, k);
    if (p.sf != T(1)) val = val * p.sf;
    const unsigned e = (unsigned)base + (unsigned)k;
    const unsigned o = g.rank(e);
    if (g.rank(e + 1u) != o) out[o] = val;                             // e lies in the box: it is output element o
  }
}


// FastDiv's windows on the host's terms (dctz_quant_host.h: divisor_in_window / value_in_window): unbiased exponent of a
// finite non-zero double in [lo, hi)
__device__ __forceinline__ bool exp_in(double v, int lo, int hi) {
  const int e = (int)(((unsigned)__double2hiint(v) >> 20) & 0x7ffu) - 1023;     // subnormal / zero: -1023, inf / NaN: 1024
  return e >= lo && e < hi;
}

}  // namespace dctz
