// dctz_kernels_fixup.hip -- the correction list: the elements whose reconstruction misses the original by more than a bound,
// built beside the streams and applied to the output of any decode (include/dctz_hip.h: dctzhip_fixup_build /
// dctzhip_fixup_apply).
//
// k_fixup_mark: k_tile_summary<T, MODE, true> with a comparison in place of the reductions.  One wave per stream tile, lane
// b = block b, grid-stride; the head is summary_tile_values (dctz_summary_head.h), so every r is bit for bit the element the
// decoders write; the original's tile arrives by the same two-phase LDS-DMA through the 16 KiB the staged coefficients have
// left.  Each phase ORs 32 comparison bits into the lane's 64-bit mask; the lane stores its mask, a wave scan of the
// popcounts gives the tile's count.
// k_fixup_mark_rem: the short last block as k_tile_summary_rem decodes it, its mask by ballot; its count joins its tile's
// behind the main kernel in stream order.
// k_fixup_scan: one level of the exclusive prefix of the tiles' counts (at most two levels for n <= INT_MAX), no atomics.
// k_fixup_emit: one wave per tile, lane b loads the mask of block b and a wave scan of the popcounts places the block; the wave
// then writes block after block, lane j the entry of element j: every entry has one place that depends on the masks alone,
// so the same call gives the same bytes whatever grid runs.
// k_fixup_apply: one wave per visited tile; the list is untrusted, so the tile's table entries and all its offsets are
// compared first and a tile that fails stores nothing; each entry is unravelled against the box and stored to the dense box.
#include "dctz_summary_head.h"

namespace dctz {

// bit j - J0 of the result: element j of the block is listed
template <typename T, int J0, int J1>
__device__ __forceinline__ unsigned fixup_compare(const T (&x)[64], const T (&o)[64], const T bound) {
  unsigned m = 0;
#pragma unroll
  for (int j = J0; j < J1; j++) m |= !(fabs(o[j] - x[j]) <= bound) ? 1u << (j - J0) : 0u;   // a NaN on either side lists the element
  return m;
}

// Waves per SIMD the register allocation of k_fixup_mark aims at.  Two, the budget of k_tile_summary's REF form: one wave
// compares while the other waits for its phase.  The fp64 QT form carries the table's lanes on top and needs a few registers
// more than the 256 that leaves, like its counterpart among the summaries: it is left to the allocator rather than spilled.
template <typename T, int MODE> struct MarkWaves { static constexpr int N = (sizeof(T) == 8 && MODE == DCTZHIP_QT) ? 1 : 2; };

template <typename T, int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MarkWaves<T, MODE>::N))) void k_fixup_mark(FixupParams<T> fp) {
  constexpr int PH = SummaryLds<T>::PH;
  using G = Geo<T, PH>;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[SummaryLds<T>::BYTES];
  const SummaryParams<T>& p = fp.s;
  float* const stage = reinterpret_cast<float*>(lds);
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  TileMap<T, PH> tm;
  tm.init(lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  bool bad = false;
  for (unsigned t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_tile_summary)
    asm volatile("" ::: "memory");
    const unsigned b0 = t * (unsigned)TILE_BLKS;
    const unsigned nblk = min(b0 + (unsigned)TILE_BLKS, p.nfull) - b0;   // the tile's whole blocks
    const bool full = (unsigned)lane < nblk;
    // the original's blocks of this tile; the range check zero-fills what lies beyond the last whole block
    const __amdgpu_buffer_rsrc_t r_ref =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p.ref + (size_t)t * TILE_ELEMS), 0, (int)(nblk * (unsigned)G::BLKB), 0x00020000);
    T x[64], o[64];
    if (!summary_tile_values<T, MODE>(p, t, lane, tab, qtl, scale, stage, x, [&] { issue_phase_dma<T, PH>(r_ref, 0u, 0, lds, tm); })) {
      bad = true;
      if (lane == 0) fp.tile_cnt[t] = 0u;
      continue;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // phase 0 has landed (and everything older is done)
    read_phase<T, PH, 0>(o, lds, tm);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // ... and is in registers before phase 1 overwrites it
    issue_phase_dma<T, PH>(r_ref, 0u, 1, lds, tm);
    const unsigned m0 = fixup_compare<T, 0, 32>(x, o, fp.bound);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    read_phase<T, PH, 1>(o, lds, tm);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // ... before the next tile's staging writes the buffer
    const unsigned m1 = fixup_compare<T, 32, 64>(x, o, fp.bound);
    const unsigned long long msk = full ? ((unsigned long long)m1 << 32) | (unsigned long long)m0 : 0ull;
    if (full) fp.mask[b0 + (unsigned)lane] = msk;
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)wave_incl_scan((unsigned)__popcll(msk)), 63);
    if (lane == 0) fp.tile_cnt[t] = tot;
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The short last block (length l = n % 64), one wave, lane k = element k
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_fixup_mark_rem(FixupParams<T> fp) {
  __shared__ T a[64], cr[128], ci[128];
  const SummaryParams<T>& p = fp.s;
  const int k = threadIdx.x;
  const int l = (int)(p.n - p.nfull * 64u);
  const size_t base = (size_t)p.nfull * 64;
  const unsigned t = p.nfull / (unsigned)TILE_BLKS;                    // the tile that holds the short block
  const bool own = (p.nfull % (unsigned)TILE_BLKS) == 0u;              // ... and nothing else: its count is this kernel's
  T val;
  if (!summary_rem_value<T, MODE>(p, k, a, cr, ci, val)) {             // (wave-uniform) refused, nothing of AC_exact read
    if (k == 0 && own) fp.tile_cnt[t] = 0u;
    return;
  }
  bool hit = false;
  if (k < l) hit = !(fabs(p.ref[base + (size_t)k] - val) <= fp.bound);
  const unsigned long long msk = __ballot(hit);
  if (k == 0) {
    fp.mask[p.nfull] = msk;
    // whole blocks in the tile: their count is the main kernel's, written in front of this launch in stream order
    fp.tile_cnt[t] = (own ? 0u : fp.tile_cnt[t]) + (unsigned)__popcll(msk);
  }
}

// One level of the exclusive prefix: workgroup g takes in[FIXUP_SCAN_WG g ...] (m values in all).
//   out (or null)    out[i] = carry[g] (or 0) + the values of the workgroup in front of i
//   sums (or null)   sums[g] = the workgroup's total
// The last workgroup knows the total -- carry[gridDim.x], or with a single workgroup and no carry its own -- and stores it
// to out[m] and to *total (each or null).
__global__ __launch_bounds__(FIXUP_SCAN_WG) void k_fixup_scan(const unsigned* __restrict__ in, const unsigned m, unsigned* __restrict__ out,
                                                             const unsigned* __restrict__ carry, unsigned* __restrict__ sums,
                                                             unsigned* __restrict__ total) {
  constexpr int NW = FIXUP_SCAN_WG / 64;
  __shared__ unsigned sh[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned i = blockIdx.x * (unsigned)FIXUP_SCAN_WG + threadIdx.x;
  const unsigned v = i < m ? in[i] : 0u;
  const unsigned incl = wave_incl_scan(v);
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  unsigned front = 0, wg = 0;
  for (int w = 0; w < NW; w++) { const unsigned s = sh[w]; front += w < wave ? s : 0u; wg += s; }
  const unsigned base = carry ? carry[blockIdx.x] : 0u;
  if (out && i < m) out[i] = base + front + incl - v;
  if (threadIdx.x == 0) {
    if (sums) sums[blockIdx.x] = wg;
    if (blockIdx.x == gridDim.x - 1 && (carry || gridDim.x == 1)) {
      const unsigned all = carry ? carry[gridDim.x] : wg;
      if (out) out[m] = all;
      if (total) *total = all;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(64) void k_fixup_emit(FixupEmitParams<T> p) {
  const int lane = threadIdx.x;
  const unsigned nblk = (p.n + 63u) / 64u;                             // the short block included
  const unsigned tiles = (p.n + (unsigned)TILE_ELEMS - 1u) / (unsigned)TILE_ELEMS;
  if (p.fix_start[tiles] > p.capacity || p.ctl->error) return;         // the list does not fit, or the masks are not all there
  const T* __restrict__ const ref = p.ref;
  uint16_t* __restrict__ const fix_off = p.fix_off;
  T* __restrict__ const fix_val = p.fix_val;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned blk = t * (unsigned)TILE_BLKS + (unsigned)lane;
    const unsigned long long msk = blk < nblk ? p.mask[blk] : 0ull;
    const unsigned c = (unsigned)__popcll(msk);
    const unsigned incl = wave_incl_scan(c);
    const unsigned tot = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
    const unsigned s0 = p.fix_start[t], s1 = p.fix_start[t + 1];
    if (s1 - s0 != tot || s1 > p.capacity) continue;                   // (never, after the scan of these masks' counts)
    // Block after block by the whole wave: lane j takes element j of block b, so the original is read in whole lines and the
    // block's entries leave as one run.  The places are the scan's: block b starts at s0 + (entries of the blocks in front).
    const unsigned at = s0 + incl - c;
    const unsigned lo = (unsigned)msk, hi = (unsigned)(msk >> 32);
    const T* const src = ref + (size_t)t * TILE_ELEMS + (size_t)lane;
    // (no branch around an empty block, and the list does not alias the original: the loads of several blocks are in flight)
#pragma unroll 8
    for (int b = 0; b < TILE_BLKS; b++) {
      const unsigned long long mb = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, b) << 32) |
                                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, b);
      const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)at, b);
      if ((mb >> lane) & 1ull) {
        const unsigned i = first + (unsigned)__popcll(mb & below);
        fix_off[i] = (uint16_t)((unsigned)b * 64u + (unsigned)lane);
        fix_val[i] = src[b * 64];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(64) void k_fixup_apply(FixupApplyParams<T> p) {
  const int lane = threadIdx.x;
  const unsigned tiles = (p.n + (unsigned)TILE_ELEMS - 1u) / (unsigned)TILE_ELEMS;
  bool bad = p.fix_start[tiles] != p.count;
  for (unsigned t = p.t0 + blockIdx.x; t < p.t1 && !bad; t += gridDim.x) {
    const unsigned e0 = t * (unsigned)TILE_ELEMS;
    const unsigned te = min((unsigned)TILE_ELEMS, p.n - e0);           // the tile's elements
    const unsigned s0 = p.fix_start[t], s1 = p.fix_start[t + 1];
    if (s1 < s0 || s1 > p.count || s1 - s0 > te) { bad = true; break; }   // (wave-uniform) every read below stays inside [0, count)
    // every offset inside the tile and above its neighbour in front, before anything is stored
    bool wrong = false;
    for (unsigned i = s0 + (unsigned)lane; i < s1; i += 64u) {
      const unsigned o = p.fix_off[i];
      wrong = wrong || o >= te || (i > s0 && (unsigned)p.fix_off[i - 1] >= o);
    }
    if (__any(wrong)) { bad = true; break; }
    for (unsigned i = s0 + (unsigned)lane; i < s1; i += 64u) {
      const unsigned e = e0 + (unsigned)p.fix_off[i];
      const unsigned o = p.box.rank(e);
      if (p.box.rank(e + 1u) != o) p.out[o] = p.fix_val[i];             // e lies in the box: it is output element o
    }
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 5u);
}

// The instantiation of a mode
template <typename T>
auto fixup_kernel(int mode) -> void (*)(FixupParams<T>) {
  using Fn = void (*)(FixupParams<T>);
  return with_mode(mode, [](auto M) -> Fn { return k_fixup_mark<T, M()>; });
}
template <typename T>
int fixup_occupancy(int mode) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fixup_kernel<T>(mode), 64, 0);
  return e == hipSuccess ? n : 0;
}
template <typename T>
void launch_fixup_mark(const FixupParams<T>& p, int mode, int grid, bool with_rem, hipStream_t s) {
  using Fn = void (*)(FixupParams<T>);
  if (grid > 0) hipLaunchKernelGGL(fixup_kernel<T>(mode), dim3(grid), dim3(64), 0, s, p);
  if (with_rem) hipLaunchKernelGGL(with_mode(mode, [](auto M) -> Fn { return k_fixup_mark_rem<T, M()>; }), dim3(1), dim3(64), 0, s, p);
}
size_t fixup_scan_slots(size_t m) {
  const size_t g = (m + FIXUP_SCAN_WG - 1) / FIXUP_SCAN_WG;
  return g > 1 ? 2 * g + 1 : 0;
}
void launch_fixup_scan(const unsigned* cnt, size_t m, unsigned* start, unsigned* part, Ctl* ctl, hipStream_t s) {
  const size_t g = (m + FIXUP_SCAN_WG - 1) / FIXUP_SCAN_WG;
  if (g <= 1) {
    hipLaunchKernelGGL(k_fixup_scan, dim3(1), dim3(FIXUP_SCAN_WG), 0, s, cnt, (unsigned)m, start, (const unsigned*)nullptr, (unsigned*)nullptr,
                       &ctl->cnt_total);
    return;
  }
  // g <= FIXUP_SCAN_WG (n <= INT_MAX: m <= 2^19): the workgroups' totals, their prefix by one workgroup, then the counts again
  unsigned* const sums = part;
  unsigned* const carry = part + g;                                    // g + 1 entries
  hipLaunchKernelGGL(k_fixup_scan, dim3((unsigned)g), dim3(FIXUP_SCAN_WG), 0, s, cnt, (unsigned)m, (unsigned*)nullptr, (const unsigned*)nullptr, sums,
                     (unsigned*)nullptr);
  hipLaunchKernelGGL(k_fixup_scan, dim3(1), dim3(FIXUP_SCAN_WG), 0, s, (const unsigned*)sums, (unsigned)g, carry, (const unsigned*)nullptr,
                     (unsigned*)nullptr, &ctl->cnt_total);
  hipLaunchKernelGGL(k_fixup_scan, dim3((unsigned)g), dim3(FIXUP_SCAN_WG), 0, s, cnt, (unsigned)m, start, (const unsigned*)carry, (unsigned*)nullptr,
                     (unsigned*)nullptr);
}
template <typename T>
void launch_fixup_emit(const FixupEmitParams<T>& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_fixup_emit<T>, dim3(grid), dim3(64), 0, s, p);
}
template <typename T>
void launch_fixup_apply(const FixupApplyParams<T>& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_fixup_apply<T>, dim3(grid), dim3(64), 0, s, p);
}
template int fixup_occupancy<double>(int);
template int fixup_occupancy<float>(int);
template void launch_fixup_mark<double>(const FixupParams<double>&, int, int, bool, hipStream_t);
template void launch_fixup_mark<float>(const FixupParams<float>&, int, int, bool, hipStream_t);
template void launch_fixup_emit<double>(const FixupEmitParams<double>&, int, hipStream_t);
template void launch_fixup_emit<float>(const FixupEmitParams<float>&, int, hipStream_t);
template void launch_fixup_apply<double>(const FixupApplyParams<double>&, int, hipStream_t);
template void launch_fixup_apply<float>(const FixupApplyParams<float>&, int, hipStream_t);

}  // namespace dctz
