// dctz_kernels_mbox.hip -- a list of boxes of one array in one call (include/dctz_hip.h: dctzhip_decompress_boxes).
//
// dctzhip_decompress_box gives every CANDIDATE tile of its box a workgroup, and most candidates of a thin or small box are
// not hit.  Here the hit test runs first, for all boxes at once: k_boxlist_build has one thread per (box, candidate tile),
// asks BoxGeo::rank at the tile's two ends -- k_decompress_box's own test -- and compacts the hits into a list of
// {box, tile} items (one ballot and one atomic add per wave).  k_decompress_mbox's single-wave workgroups then take items
// w, w + G, ... of that list, up to the count the builder left in device memory: every workgroup decodes hit tiles only, the
// host is not asked in between.  Per item the record of the box is read by wave-uniform loads, and the tile is
// k_decompress_box's (box_tile_scatter below) into the record's output.  The order of the list is free --
// the output positions of an item follow from rank() alone.
// The short last block is k_decompress_mbox_rem's, one workgroup per box that reaches into it (the host knows which).
#include "dctz_kernel_common.h"

namespace dctz {

// One thread per (box, candidate); `unit` is what a candidate spans in the units g.rank counts in, `end` where the last
// candidate ends.  Never stores at or beyond p.cap: a count above it sets error = 4 instead (the host's bound was wrong).
__global__ __launch_bounds__(256) void k_boxlist_build(BoxListParams p) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  bool hit = false;
  unsigned b = 0, t = 0;
  if (gid < p.total) {
    unsigned hi = p.nbox;                                              // the last record with cand0 <= gid
    while (hi - b > 1u) {
      const unsigned mid = (b + hi) >> 1;
      if (p.recs[mid].cand0 <= gid) b = mid; else hi = mid;
    }
    const BoxRec& r = p.recs[b];
    t = r.t0 + (gid - r.cand0);
    const unsigned ts = t * p.unit;
    const unsigned te = min(ts + p.unit, p.end);
    hit = r.g.rank(ts) != r.g.rank(te);
  }
  const unsigned long long mask = __ballot(hit);
  if (mask == 0ull) return;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned cnt = (unsigned)__popcll(mask);
  unsigned base = 0;
  if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(&p.ctl->cnt_total, cnt);
  base = (unsigned)__builtin_amdgcn_readlane((int)base, __ffsll((long long)mask) - 1);
  if (base + cnt > p.cap && lane == 0) atomicExch(&p.ctl->error, 4u);
  const unsigned at = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  if (hit && at < p.cap) p.items[at] = BoxItem{b, t};
}

// a record into scalar registers, word by word (every lane reads the same address)
__device__ __forceinline__ BoxRec uniform_rec(const BoxRec* r) {
  struct Words { unsigned w[sizeof(BoxRec) / 4]; } v;
  const unsigned* s = reinterpret_cast<const unsigned*>(r);
#pragma unroll
  for (unsigned i = 0; i < sizeof(BoxRec) / 4; i++) v.w[i] = (unsigned)__builtin_amdgcn_readfirstlane((int)s[i]);
  return __builtin_bit_cast(BoxRec, v);
}

// A hit tile of a box: tile t = flat elements [ts, te), oa = g.rank(ts), oe = g.rank(te), oe != oa.  This is the text of
// k_decompress_box's loop body (dctz_kernels_box.hip) from its ra_tile_image call to its closing barrier, with g and out in
// place of the launch constants.  It is a COPY: with one function called from both kernels the four k_decompress_box
// instantiations came out with other register counts than before (EXPERIMENTS.md, "Many boxes in one call"), and that
// kernel's text stays as it was measured.  A change to either belongs in both.
// False: ra_tile_image's (nothing was stored).  g and out are wave-uniform.
template <typename T, int MODE, typename P>
__device__ __forceinline__ bool box_tile_scatter(const P& p, const BoxGeo& g, T* const out, const unsigned t, const unsigned ts,
                                                 const unsigned te, const unsigned oa, const unsigned oe, const unsigned full_end,
                                                 const int lane, const CTab<T> tab, const QtLanes<T>& qtl, const bool scale,
                                                 unsigned char* lds) {
  using G = RaGeo<T>;
  const T* const img = reinterpret_cast<const T*>(lds);
  if (!ra_tile_image<T, MODE>(p, t, lane, tab, qtl, scale, lds)) return false;
  // the tile's whole-block elements inside the box -> out[oa, ob)
  const unsigned ob = te > full_end ? g.rank(max(full_end, ts)) : oe;
  if (oa < ob) {
    // (a descriptor per tile: out[oa, ob) and not a byte more -- num_records is 32 bits, a box may be larger)
    const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(out + oa, 0, (int)((ob - oa) * sizeof(T)), 0x00020000);
    unsigned o = oa + (unsigned)lane;
    if (o < ob) {
      unsigned b[BOX_ND];
      unsigned f = g.flat_of(o, b);
      for (;;) {
        const T v = img[G::at(f - ts)];
        const int at = (int)((o - oa) * (unsigned)sizeof(T));
        if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r_out, at, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r_out, at, 0, 0);
        o += 64u;
        if (o >= ob) break;
        unsigned carry = 0, df = g.fstep;
#pragma unroll
        for (int d = BOX_ND - 1; d > 0; d--) {                         // b + step < 2 ext: one carry per dimension
          b[d] += g.step[d] + carry;
          carry = b[d] >= g.ext[d] ? 1u : 0u;
          b[d] -= carry ? g.ext[d] : 0u;
          df += carry ? g.wrap[d] : 0u;
        }
        f += df;
      }
    }
  }
  __syncthreads();                                                     // the image is read out before the next tile's staging
  return true;
}

template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_mbox(MBoxParams<T> p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[RaGeo<T>::BYTES];
  const int lane = threadIdx.x;
  const CTab<T> tab = as_ctab<T>(p.tab);
  QtLanes<T> qtl{};
  if (MODE == DCTZHIP_QT) qtl.load(p.qtab, lane);
  const bool scale = (p.sf != T(1));                                   // dctz-decomp-lib.c:496 / :505
  const unsigned full_end = p.nfull * 64u;
  const unsigned count = min((unsigned)__builtin_amdgcn_readfirstlane((int)p.ctl->cnt_total), p.cap);
  bool bad = false;
  for (unsigned i = blockIdx.x; i < count; i += gridDim.x) {
    // (a compiler barrier per trip: keeps the transform's scalar constant loads inside the loop, as in k_rd_probe)
    asm volatile("" ::: "memory");
    const unsigned b = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].box);
    const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)p.items[i].tile);
    const BoxRec rec = uniform_rec(p.recs + b);
    const unsigned ts = t * (unsigned)TILE_ELEMS;
    const unsigned te = min(ts + (unsigned)TILE_ELEMS, p.n);
    const unsigned oa = rec.g.rank(ts);
    const unsigned oe = rec.g.rank(te);
    if (!box_tile_scatter<T, MODE>(p, rec.g, static_cast<T*>(rec.out), t, ts, te, oa, oe, full_end, lane, tab, qtl, scale, lds)) bad = true;
  }
  if (bad && lane == 0) atomicExch(&p.ctl->error, 2u);
}

// The short last block, workgroup w for box rem_boxes[w]: k_decompress_box_rem with the record in place of the launch
// constants.
template <typename T, int MODE>
__global__ __launch_bounds__(64) void k_decompress_mbox_rem(MBoxParams<T> p) {
  __shared__ T a[64];
  __shared__ T cr[128];
  __shared__ T ci[128];
  const BoxRec rec = uniform_rec(p.recs + p.rem_boxes[blockIdx.x]);
  box_rem_block<T, MODE>(p, rec.g, static_cast<T*>(rec.out), (int)threadIdx.x, a, cr, ci);
}

void launch_boxlist_build(const BoxListParams& p, hipStream_t s) {
  hipLaunchKernelGGL(k_boxlist_build, dim3((p.total + 255u) / 256u), dim3(256), 0, s, p);
}

template <typename T>
auto mbox_kernel(int mode) -> void (*)(MBoxParams<T>) {
  return with_mode(mode, [](auto M) { return k_decompress_mbox<T, M()>; });
}
template <typename T>
int mbox_occupancy(int mode) {
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mbox_kernel<T>(mode), 64, 0);
  return e == hipSuccess ? n : 0;
}

template <typename T>
void launch_decompress_mbox(const MBoxParams<T>& p, int mode, int grid, int nrem, hipStream_t s) {
  hipLaunchKernelGGL(mbox_kernel<T>(mode), dim3(grid), dim3(64), 0, s, p);
  if (nrem > 0) hipLaunchKernelGGL(with_mode(mode, [](auto M) { return k_decompress_mbox_rem<T, M()>; }), dim3(nrem), dim3(64), 0, s, p);
}
template int mbox_occupancy<double>(int);
template int mbox_occupancy<float>(int);
template void launch_decompress_mbox<double>(const MBoxParams<double>&, int, int, int, hipStream_t);
template void launch_decompress_mbox<float>(const MBoxParams<float>&, int, int, int, hipStream_t);

}  // namespace dctz
