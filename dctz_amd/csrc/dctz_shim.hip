// dctz_shim.hip -- the C ABI of include/dctz_hip.h over the gfx950 kernels.
//
// Host-side responsibilities only: argument checking, scratch management,
// the libm expressions the reference evaluates on the host (scaling factor
// util.c:29/43, bin ranges dctz-comp-lib.c:271-281, twiddle tables
// dct.c:37-47/130-134), kernel sequencing on one HIP stream, and reading back
// the few scalars the host stage needs (cnt, QT table).  No CPU compute path
// exists: if HIP is unavailable every call returns DCTZHIP_E_HIP.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <chrono>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "dctz_device.h"
#include "dctz_tables.h"
#include "dctz_spec_memory.h"
#include "dctz_quant_host.h"

// RCCL is loaded with dlopen (single-GPU users need none), so its header is not needed -- but where it is installed at build
// time, the things this file restates from it are checked against it by the compiler (the header declares, it defines
// nothing: no link dependency); at load time the library's major version is checked (rccl_load).
#define DCTZ_NCCL_UINT8 1
#define DCTZ_NCCL_UINT64 5
#define DCTZ_NCCL_FLOAT32 7
#if defined(__has_include)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
static_assert(sizeof(ncclUniqueId) == DCTZHIP_COMM_ID_BYTES, "DCTZHIP_COMM_ID_BYTES must be sizeof(ncclUniqueId) of the installed RCCL");
static_assert((int)ncclUint8 == DCTZ_NCCL_UINT8 && (int)ncclUint64 == DCTZ_NCCL_UINT64 && (int)ncclFloat32 == DCTZ_NCCL_FLOAT32,
              "ncclDataType_t values differ from the installed rccl.h");
static_assert(NCCL_MAJOR == 2, "this file was written against the NCCL 2 API");
#endif
#endif

using namespace dctz;

struct dctzhip_ctx {
  int device = 0;
  int num_cu = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t side_stream = nullptr;   // serial-order mean, runs beside the host zlib tail
  hipEvent_t serial_ev = nullptr;      // ... behind what is queued on `stream` when dctzhip_serial_mean_begin is called
  double* serial_out = nullptr;
  size_t serial_n = 0;
  int serial_dtype = -1;
  // constant tables
  double* tab_f64 = nullptr;
  float* tab_f32 = nullptr;
  void* rtab = nullptr;             // RTAB_SIZE doubles (either dtype)
  int rtab_l = -1, rtab_dtype = -1;
  void* qtab = nullptr;             // 64 doubles
  // per-call state
  Ctl* ctl = nullptr;               // the control block of the current call: one of ctl_pair's two
  Ctl* ctl_pair = nullptr;          // a compress call that guesses sf from spec_mem moves to the other block, which the hand-off workgroup of the last k_compact_ac has zeroed: no launch in front of k_compress
  int ctl_other_clean = 0;          // the block c->ctl is NOT is all zeros (the hand-off of the call that zeroed it has been seen, nothing has used it since)
  double* part = nullptr;           // stats partials
  double* stats_out = nullptr;      // 4 doubles
  float* ac_tmp = nullptr;          // workgroup-local AC_exact lists (list of workgroup b at the slot of its first tile)
  size_t ac_tmp_cap = 0;            // floats
  unsigned* tile_cnt = nullptr;     // list lengths (compress) / per-tile flag counts (decode) and their exclusive prefix
  unsigned* wg_cnt = nullptr;       // decode: flag counts per workgroup of k_decompress
  size_t tile_cap = 0;              // entries
  unsigned* qcnt = nullptr;         // k_compress -> k_compact_ac: per block, the counts of its tile's sub-lists (dctz_device.h: Sub)
  unsigned* ttot = nullptr;         // ... per tile, its "stored exactly" coefficients
  unsigned* tile_pre = nullptr;     // decode, tile-interleaved k_decompress: per tile, the counts of its range's tiles in front of it
  // Decode memo.  A compress call on the chain of kernels leaves, beside ttot[] (every tile's count of exact coefficients),
  // memo_start[]: every tile's first place in AC_exact[] (k_compact_ac).  `memo` names the streams those tables describe; a
  // dctzhip_decompress of exactly these streams takes the tables in place of k_count_tiles' pass over bin_index, and the
  // decoder checks every count against the flags it reads anyway (dctz_kernels.hip: k_decompress_il, MEMO).  Per tile and
  // absolute: the partitions of the two sides do not matter.
  unsigned* memo_start = nullptr;   // (allocated with ttot)
  struct DecodeMemo {
    bool valid = false;
    const void* bin = nullptr; const void* dc = nullptr; const void* ac = nullptr;
    size_t n = 0;
    int dtype = 0, mode = 0;
    unsigned cnt_total = 0;
    hipStream_t stream = nullptr;
  } memo;
  bool memo_pass = false;           // the last compress_pass filled both tables (flat blocks through k_compress + k_compact_ac)
  int dec_memo = 1;                 // 0: every decode counts its flags first (DCTZHIP_DEC_MEMO, dctzhip_set_decode_memo)
  unsigned long long memo_decodes = 0, memo_redos = 0;   // decodes launched on the memo / of them found stale and done again (dctzhip_debug_counter 16 / 17)
  unsigned* ix_part = nullptr;      // dctzhip_ac_index: flag counts per workgroup of k_ac_index, then their exclusive prefix
  size_t ix_part_cap = 0;           // entries
  int ra_occ[2][2] = {{0, 0}, {0, 0}};   // dctzhip_decompress_range: resident workgroups per CU of k_decompress_range [fp64][QT] on this device (0: not asked yet)
  int box_occ[2][2] = {{0, 0}, {0, 0}};  // dctzhip_decompress_box: the same of k_decompress_box
  int ndbox_occ[2][2][2] = {};      // dctzhip_decompress_box_nd: the same of k_decompress_ndbox, [fp64][QT][3-D]
  int sum_occ[2][2][3][2] = {};     // dctzhip_tile_summary / _nd: the same of k_tile_summary / k_ndsummary, [fp64][QT][geometry][with an original]
  dctzhip_tile_summary_t* sum_buf = nullptr;   // ... the levels of k_tile_summary_final, then the records of a call without d_tiles
  size_t sum_cap = 0;               // records
  int fix_occ[2][2][3] = {};        // dctzhip_fixup_build / _nd: the same of k_fixup_mark / k_ndfix_mark, [fp64][QT][geometry]
  unsigned long long* fix_mask = nullptr;   // ... a mask per block of the array
  size_t fix_mask_cap = 0;          // words
  unsigned* fix_cnt = nullptr;      // ... a count per tile, then the levels of k_fixup_scan
  size_t fix_cnt_cap = 0;           // entries
  void* mask_filled = nullptr;      // dctzhip_compress_masked without d_filled: the filled copy
  size_t mask_filled_cap = 0;       // bytes
  int coarse_occ[2][2][3][5] = {};  // dctzhip_decompress_coarse / _coarse_nd: the same of k_decompress_coarse / _coarse_nd, [fp64][QT][geometry][log2 K - 1]
  int ndcbox_occ[2][2][2][2] = {};  // dctzhip_decompress_coarse_box_nd: the same of k_ndcoarse_box, [fp64][QT][3-D][K == 4]
  unsigned box_grid = 0, box_tiles = 0;  // the last box call (_box, _box_nd, _coarse_box_nd): workgroups launched, candidate tiles (dctzhip_debug_counter 11 / 12)
  // dctzhip_decompress_boxes: the box table (records, then the boxes of the short block) in pinned host memory and on the
  // device, the list of hit (box, tile) items, resident workgroups per CU of k_decompress_mbox [fp64][QT]
  unsigned char* mb_pin = nullptr;
  unsigned char* mb_dev = nullptr;
  BoxItem* mb_items = nullptr;
  size_t mb_items_cap = 0;          // items
  int mbox_occ[2][2] = {{0, 0}, {0, 0}};
  int mboxnd_occ[2][2][2] = {};     // dctzhip_decompress_boxes_nd: the same of k_decompress_mbox_nd, [fp64][QT][3-D]; table, list and counters are shared
  int mcboxnd_occ[2][2][2][2] = {}; // dctzhip_decompress_coarse_boxes_nd: the same of k_ndcoarse_mbox, [fp64][QT][3-D][K == 4]; shared likewise
  unsigned mbox_items = 0, mbox_grid = 0, mbox_bound = 0;   // ... its last call: items listed, workgroups of the decode launch, the bound B (dctzhip_debug_counter 13 / 14 / 15)
  int dec_il = 1;                   // 0: k_decompress with a contiguous tile range per workgroup; 1: interleaved for fp64 EC; 2: for all (DCTZHIP_DEC_IL)
  size_t qcnt_cap = 0;              // tiles the two hold
  void* qt_item = nullptr;
  uint8_t* qt_j = nullptr;
  size_t qt_cap = 0;                // bytes of qt_item
  size_t qtj_cap = 0;
  // device-side choice of the scaling factor for speculative calls (dctz_device.h: SfGuess / SfTable)
  double* sf_thr[2] = {nullptr, nullptr};   // [DCTZHIP_F32], [DCTZHIP_F64]
  double* sf_pw[2] = {nullptr, nullptr};
  int sf_nk[2] = {0, 0};
  SfGuess* sf_guess = nullptr;
  int dev_sf = 1;                   // 0: the host chooses sf between the sample and k_compress (DCTZHIP_DEVICE_SF)
  int blocking = 0;                 // 1: every compress / decompress call ends with a stream synchronisation (DCTZHIP_BLOCKING, dctzhip_set_blocking)
  int occ[2][2][2][2][3] = {};      // resident workgroups per CU per kernel instantiation [f64][decode][qt][stats][geom], 0 = not asked yet
  int eo = 0;                       // 1: flat fp64 arrays on the chain of kernels go through k_compress_eo (a block over two lanes; DCTZHIP_EO, dctzhip_set_split)
  int eo_occ[2][4] = {};            // its resident workgroups per CU [qt][stats + 2 * direct]
  unsigned long long eo_calls = 0;
  int eo_direct = 0;                // with k_compress_eo in EC mode: AC_exact placed in the same pass (look-back over the tiles' counts), no k_compact_ac (DCTZHIP_EO_DIRECT, dctzhip_set_split(ctx, 3)); measured slower than the lists (round 5: 356 against 261 us at p = 5 %), hence off
  int eo_lb_fail = 0;               // (tests) the look-back of one tile reports that it gave up (DCTZHIP_EO_LB_FAIL)
  int eo_direct_pause = 0;          // calls left on the lists after a look-back that gave up
  unsigned long long eo_direct_calls = 0, eo_lb_fallbacks = 0;
  unsigned long long* lb_desc = nullptr;   // per-tile descriptors of the look-back (zeroed when allocated, tagged by lb_epoch)
  unsigned* lb_ticket = nullptr;    // 8 ticket counters, 16 words apart; zero between calls (k_finish clears them)
  size_t lb_cap = 0;
  unsigned lb_epoch = 0;
  int grid_c = 0;                   // upper bound of k_compress's grid (DCTZHIP_GRID_C; 0 = what the LDS admits)
  int nd_direct = 1;                // multi-dimensional blocks read / written in place where the shape allows (DCTZHIP_ND_DIRECT)
  // large D2H copies into pageable memory: pinned staging slots, one per worker thread, each with its own stream
  static constexpr int STAGE_WORKERS = 8;
  static constexpr size_t STAGE_SLOT = (size_t)16 << 20;
  void* stage[STAGE_WORKERS] = {};
  hipStream_t stage_stream[STAGE_WORKERS] = {};
  int staged_d2h = 1;               // 0: one hipMemcpy (DCTZHIP_STAGED_D2H)
  hipEvent_t dfl_ev = nullptr;
  int dfl_side = 1;                 // 0: the sections of a dctzhip_deflate call one after the other on one stream (DCTZHIP_DEFLATE_SIDE)
  void* dfl_buf = nullptr;          // GPU entropy stage: chunk slots, sizes, offsets (dctz_deflate.hip)
  size_t dfl_cap = 0;               // bytes
  unsigned long long* dfl_len = nullptr;      // stream lengths of up to 8 sections (pinned host memory the kernels write)
  unsigned long long* dfl_len_dev = nullptr;
  void* nd_buf = nullptr;           // multi-dimensional blocks: the array laid out block after block (k_gather_nd / k_scatter_nd)
  size_t nd_cap = 0;                // bytes
  // pinned host staging
  unsigned char* h_pin = nullptr;   // [0,64): stats, [64, 64+sizeof(Ctl)): ctl, then tables
  HostBox* box = nullptr;           // result mailbox, fine-grained pinned host memory (kernels write, host spins)
  HostBox* box_dev = nullptr;       // the same memory as the device sees it
  unsigned long long seq = 0;       // sequence number of the last hand-off
  int handoff = 1;                  // 1: mailbox + spin; 0: D2H copy + hipStreamSynchronize (DCTZHIP_HANDOFF)
  int ctl_dirty = 1;                // control block may be non-zero: memset it before the next call
  // profiling
  int fuse_scaled = 1;              // d_scaled (out of place, flat blocks) written by k_compress itself instead of a k_scale pass (DCTZHIP_FUSE_SCALED)
  int fastdiv = 2;                  // hoisted-reciprocal division: 0 off, 1 per-tile window test, 2 + skip the test when k_stats proves it (DCTZHIP_FASTDIV)
  int stats_grid = 2048;            // workgroups of the statistics kernel (DCTZHIP_STATS_GRID, <= 2048)
  int wg_per_cu = 0;                // grid = CUs * this; 0 = as many single-wave workgroups as a CU's LDS admits (DCTZHIP_WG_PER_CU)
  int speculate = 1;                // fused statistics behind a sampled guess of the scaling factor (DCTZHIP_SPECULATE, dctzhip_set_speculation)
  size_t spec_min = (size_t)1 << 22; // elements below which the plain statistics pass is kept (DCTZHIP_SPEC_MIN)
  unsigned spec_group = 64;         // one 4 KiB chunk sampled per group of this many (DCTZHIP_SPEC_GROUP)
  int spec_cooldown = 0;            // calls left without speculation after a wrong guess
  int batch_speculate = 1;          // ... and in the batch sequences, for items from spec_min elements on (DCTZHIP_BATCH_SPECULATE)
  int b_spec_now = 0;               // this batch call may speculate (no cooldown pending when it started)
  unsigned long long b_spec_items = 0, b_spec_misses = 0;   // speculative batch items / those done again on their own
  unsigned long long spec_hits = 0, spec_misses = 0;
  SpecMemory spec_mem;              // the last verified statistics per (input, length, element type): a guess that needs no sample (dctz_spec_memory.h)
  int spec_memory = 1;              // 0: every speculative call samples (DCTZHIP_SPEC_MEMORY, dctzhip_set_spec_memory)
  unsigned long long hist_hits = 0, hist_misses = 0;   // guesses taken from spec_mem that verified / that did not (dctzhip_debug_counter 18 / 19)
  unsigned pass_fast_bw = 0;        // FwdParams::fast_bw of the last compress_pass / compress_one launch
  unsigned variant = 0;             // fast_sf | fast_bw << 8 of the last verified pass of a single-array compress call (dctzhip_debug_counter 20)
  int profiling = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  dctzhip_timings last = {0, 0, 0, 0};
  int have_timings = 0;
  // multi-GPU gather (RCCL, loaded on first use)
  void* comm = nullptr;             // ncclComm_t
  int comm_rank = 0, comm_world = 0;
  unsigned long long* comm_sizes_dev = nullptr;   // 3 * world u64 (all-gather target) + 3 (this rank's)
  // batches (dctzhip_compress_batch / dctzhip_decompress_batch): per-array control blocks, device-chosen scaling factors
  // and statistics; the item table (pinned host copy the first kernel reads + the device copy the others read); results
  Ctl* b_ctl = nullptr;
  SfGuess* b_guess = nullptr;
  double* b_stats = nullptr;        // 3 per array
  unsigned* b_remcnt = nullptr;     // decode: flags of every array's remainder block
  size_t b_cap = 0;                 // arrays the four buffers above hold
  int b_ctl_dirty = 1;
  unsigned char* b_blob = nullptr;  // fine-grained pinned host memory
  unsigned char* b_blob_hdev = nullptr;   // ... as the device sees it
  unsigned char* b_blob_dev = nullptr;
  size_t b_blob_cap = 0;
  unsigned char* b_res = nullptr;   // results (fine-grained pinned host memory): BatchResC | BatchResD per array, then BatchResQ per array
  unsigned char* b_res_hdev = nullptr;
  size_t b_res_cap = 0;
  void* rtab_cache[2][64] = {};     // remainder-block tables per (dtype, length), device
  // one launch per call (dctz_kernels_one.hip): the board of granules, the control blocks of this and the next such call
  unsigned long long* one_ga = nullptr;
  unsigned long long* one_gb = nullptr;
  double* one_rec = nullptr;
  Ctl* one_ctl = nullptr;           // three blocks: compress calls alternate between [0] and [1] (a call's hand-off zeroes the other one); [2]: decode's error word
  unsigned one_cslot = 0;
  unsigned long long* one_qt = nullptr;    // QT: two tables of per-position maxima (this call's, the next call's), ONE_QT_WORDS each
  unsigned long long* one_bqt = nullptr;   // ... of a batch: two halves of one_bctl_cap x 64 words
  int one_bad_guess = 0;            // DCTZHIP_ONE_BADGUESS (tests): 1 = the replay path of k_compress_one on every call, 3 = it guesses whatever the grid
  unsigned long long* one_dbg = nullptr;   // DCTZHIP_ONE_STAMPS=1: 16 time stamps per workgroup of the last one-launch kernel
  unsigned one_epoch = 0;
  int one = 1;                      // 0: always the chain of kernels (DCTZHIP_ONE)
  int one_cooldown = 0;             // calls left on the chain after a launch whose workgroups were not all resident
  int one_occ[2][2][2][2] = {};     // resident workgroups per CU [f64][decode][qt][scaled], 0 = not asked yet
  unsigned long long one_calls = 0, one_fallbacks = 0;
  char last_kernel[6][96] = {};     // the big kernel launched last, as rocprofv3 lists it: [0] compress, [1] decompress, [2] / [3] batch compress f64 / f32, [4] / [5] batch decompress (dctzhip_debug_last_kernel)
  int one_withhold = 0;             // (tests: dctzhip_debug_knob) workgroup 0 of a one-launch kernel withholds its granule
  Ctl* one_bctl = nullptr;          // batches through the one-launch kernels: two halves of one_bctl_cap control blocks (this call's, the next call's)
  size_t one_bctl_cap = 0;
  unsigned one_bslot = 0, one_bdirty[2] = {0, 0};   // half of the next call; leading entries of a half that may be non-zero
  int b_one_seen[2] = {0, 0};       // element types of the current batch call that went through the one-launch kernels (profiling)
  hipStream_t b_stream = nullptr;   // a mixed batch runs its fp32 sequences here, beside the fp64 ones on the context's stream
  hipEvent_t b_fork = nullptr, b_join = nullptr;
  hipEvent_t b_ev[2][5] = {};       // profiling: per element-type sequence of the last batch call
  dctzhip_timings b_last[2] = {};
  int b_have_timings = 0;
  // rate-distortion probe and target-PSNR compression (dctzhip_rd_probe / dctzhip_compress_psnr)
  double* rd_slab = nullptr;        // k_rd_probe's workgroup rows, then 64 doubles of bound constants and 64 of results
  size_t rd_slab_cap = 0;           // doubles
  void* rd_rec = nullptr;           // dctzhip_compress_psnr: the decoded array it measures (n elements)
  size_t rd_rec_cap = 0;            // bytes
  int rd_sse_div = 1;               // (tests: dctzhip_debug_knob 3) every predicted SSE is divided by this
  unsigned long long rd_stepdowns = 0;   // dctzhip_compress_psnr: measured misses that stepped to the next smaller bound
  char err[512] = {0};
};

static char g_create_err[512] = "";
static int build_sf_tables(dctzhip_ctx* c);
static constexpr int STATS_GRID_MAX = 2048;
static constexpr int PART_SLOTS = 256 * 16 + 64;       // >= largest k_compress grid + 1 (fused statistics partials), >= 4/3 of the PSNR grid
static constexpr int SPEC_COOLDOWN = 8;
static constexpr int ONE_BOARD = 256 * 8 + 64;         // granules of the one-launch path: workgroups of ONE_TW waves, at most 8 per CU
static constexpr int ONE_COOLDOWN = 64;
static constexpr unsigned ONE_QT_SHARDS = 4, ONE_QT_STRIDE = 32;      // single arrays: a word per 256 bytes, four shards (dctz_device.h: OneFwd::qt)
static constexpr size_t ONE_QT_WORDS = (size_t)ONE_QT_SHARDS * 64 * ONE_QT_STRIDE;
static constexpr int WG_PER_CU_MAX = 12;               // single-wave workgroups per CU: three per SIMD (k_compress<float>: 160 VGPRs, 12 KiB of LDS)
static constexpr size_t PIN_STATS = 0, PIN_CTL = 64, PIN_TAB = 64 + sizeof(Ctl);
static constexpr size_t PIN_BYTES = PIN_TAB + sizeof(double) * RTAB_SIZE + sizeof(double) * 64;

static int fail(dctzhip_ctx* c, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(c ? c->err : g_create_err, 512, fmt, ap);
  va_end(ap);
  return code;
}

#define HIPCHK(c, call)                                                                         \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail((c), DCTZHIP_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" const char* dctzhip_version(void) { return "0.4.0"; }

extern "C" const char* dctzhip_last_error(const dctzhip_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

extern "C" int dctzhip_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int dctzhip_ctx_create(dctzhip_ctx** out, int device) {
  if (!out) return fail(nullptr, DCTZHIP_E_ARG, "dctzhip_ctx_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  HIPCHK(nullptr, hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(nullptr, DCTZHIP_E_HIP, "no HIP device visible (this library has no CPU path)");
  if (device < 0) HIPCHK(nullptr, hipGetDevice(&device));
  if (device >= ndev) return fail(nullptr, DCTZHIP_E_ARG, "device %d out of range (%d visible)", device, ndev);
  HIPCHK(nullptr, hipSetDevice(device));
  dctzhip_ctx* c = new dctzhip_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char* e = getenv("DCTZHIP_FASTDIV")) c->fastdiv = atoi(e);
  if (const char* e = getenv("DCTZHIP_FUSE_SCALED")) c->fuse_scaled = atoi(e);
  if (const char* e = getenv("DCTZHIP_STATS_GRID")) { int v = atoi(e); if (v >= 1 && v <= STATS_GRID_MAX) c->stats_grid = v; }
  if (const char* e = getenv("DCTZHIP_WG_PER_CU")) { int v = atoi(e); if (v >= 1 && v <= WG_PER_CU_MAX) c->wg_per_cu = v; }
  if (const char* e = getenv("DCTZHIP_SPECULATE")) c->speculate = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_BATCH_SPECULATE")) c->batch_speculate = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_SPEC_MIN")) { long long v = atoll(e); if (v >= 0) c->spec_min = (size_t)v; }
  if (const char* e = getenv("DCTZHIP_SPEC_MEMORY")) c->spec_memory = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_SPEC_GROUP")) { int v = atoi(e); if (v >= 1 && v <= 4096) c->spec_group = (unsigned)v; }
  HIPCHK(nullptr, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  HIPCHK(nullptr, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
  HIPCHK(nullptr, hipMalloc(&c->serial_out, 16));
  HIPCHK(nullptr, hipMalloc(&c->tab_f64, sizeof(double) * TBP_TOTAL));
  HIPCHK(nullptr, hipMalloc(&c->tab_f32, sizeof(float) * TBP_TOTAL));
  HIPCHK(nullptr, hipMalloc(&c->rtab, sizeof(double) * RTAB_SIZE));
  HIPCHK(nullptr, hipMalloc(&c->qtab, sizeof(double) * 64));
  HIPCHK(nullptr, hipMalloc(&c->ctl_pair, sizeof(Ctl) * 2));
  c->ctl = c->ctl_pair;
  HIPCHK(nullptr, hipMalloc(&c->part, sizeof(double) * 3 * PART_SLOTS * 2));      // (second half: the second chain of a mixed batch)
  HIPCHK(nullptr, hipMalloc(&c->stats_out, sizeof(double) * 4));
  HIPCHK(nullptr, hipHostMalloc(&c->h_pin, PIN_BYTES, hipHostMallocDefault));
  // the mailbox needs fine-grained (coherent) pinned host memory that kernels can write; where the
  // platform cannot provide it the library falls back to D2H copies + stream synchronisation
  if (hipHostMalloc(reinterpret_cast<void**>(&c->box), sizeof(HostBox), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess &&
      hipHostGetDevicePointer(reinterpret_cast<void**>(&c->box_dev), c->box, 0) == hipSuccess) {
    memset(c->box, 0, sizeof(HostBox));
  } else {
    (void)hipGetLastError();
    if (c->box) { (void)hipHostFree(c->box); c->box = nullptr; }
    c->box_dev = nullptr;
    c->handoff = 0;
  }
  if (const char* e = getenv("DCTZHIP_HANDOFF")) c->handoff = (atoi(e) != 0) && c->box != nullptr;
  {
    double t64[TBP_TOTAL];
    float t32[TBP_TOTAL];
    fill_tab_block<double>(t64);
    fill_tab_block<float>(t32);
    HIPCHK(nullptr, hipMemcpy(c->tab_f64, t64, sizeof(t64), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(c->tab_f32, t32, sizeof(t32), hipMemcpyHostToDevice));
  }
  for (int i = 0; i < 6; i++) HIPCHK(nullptr, hipEventCreate(&c->ev[i]));
  if (const char* e = getenv("DCTZHIP_DEVICE_SF")) c->dev_sf = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_ND_DIRECT")) c->nd_direct = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_GRID_C")) c->grid_c = atoi(e);
  if (const char* e = getenv("DCTZHIP_EO")) c->eo = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_EO_DIRECT")) c->eo_direct = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_EO_LB_FAIL")) c->eo_lb_fail = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_BLOCKING")) c->blocking = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_STAGED_D2H")) c->staged_d2h = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_DEC_MEMO")) c->dec_memo = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_DEC_IL")) c->dec_il = atoi(e);      // 0: never, 1: where it measured faster (fp64 EC), 2: every element type and mode
  if (const char* e = getenv("DCTZHIP_DEFLATE_SIDE")) c->dfl_side = atoi(e) != 0;
  if (int rc = build_sf_tables(c)) return rc;
  if (const char* e = getenv("DCTZHIP_ONE")) c->one = atoi(e) != 0;
  if (const char* e = getenv("DCTZHIP_ONE_BADGUESS")) c->one_bad_guess = atoi(e);
  HIPCHK(nullptr, hipMalloc(&c->one_ga, sizeof(unsigned long long) * ONE_BOARD));
  HIPCHK(nullptr, hipMalloc(&c->one_gb, sizeof(unsigned long long) * ONE_BOARD));
  HIPCHK(nullptr, hipMalloc(&c->one_rec, sizeof(double) * 3 * ONE_BOARD));
  HIPCHK(nullptr, hipMalloc(&c->one_ctl, sizeof(Ctl) * 3));
  HIPCHK(nullptr, hipMemset(c->one_ga, 0, sizeof(unsigned long long) * ONE_BOARD));
  HIPCHK(nullptr, hipMemset(c->one_gb, 0, sizeof(unsigned long long) * ONE_BOARD));
  HIPCHK(nullptr, hipMemset(c->one_ctl, 0, sizeof(Ctl) * 3));
  HIPCHK(nullptr, hipMalloc(&c->one_qt, sizeof(unsigned long long) * 2 * ONE_QT_WORDS));
  HIPCHK(nullptr, hipMemset(c->one_qt, 0, sizeof(unsigned long long) * 2 * ONE_QT_WORDS));
  if (const char* e = getenv("DCTZHIP_ONE_STAMPS")) if (atoi(e)) { HIPCHK(nullptr, hipMalloc(&c->one_dbg, sizeof(unsigned long long) * 16 * ONE_BOARD)); HIPCHK(nullptr, hipMemset(c->one_dbg, 0, sizeof(unsigned long long) * 16 * ONE_BOARD)); }
  *out = c;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_comm_destroy(dctzhip_ctx* c);
extern "C" void dctzhip_ctx_destroy(dctzhip_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)dctzhip_comm_destroy(c);
  (void)hipStreamSynchronize(c->stream);
  if (c->side_stream) { (void)hipStreamSynchronize(c->side_stream); (void)hipStreamDestroy(c->side_stream); }
  void* bufs[] = {c->tile_pre, c->ix_part, c->one_qt, c->one_bqt, c->one_bctl, c->one_dbg, c->one_ga, c->one_gb, c->one_rec, c->one_ctl, c->qcnt, c->ttot, c->memo_start, c->ac_tmp, c->tile_cnt, c->wg_cnt, c->serial_out, c->tab_f64, c->tab_f32, c->rtab, c->qtab, c->ctl_pair, c->part, c->stats_out, c->qt_item, c->qt_j, c->nd_buf, c->dfl_buf, c->sf_thr[0], c->sf_thr[1], c->sf_pw[0], c->sf_pw[1], c->sf_guess, c->rd_slab, c->rd_rec, c->mb_dev, c->mb_items, c->sum_buf, c->fix_mask, c->fix_cnt, c->mask_filled, c->lb_desc, c->lb_ticket};
  for (void* b : bufs) if (b) (void)hipFree(b);
  if (c->h_pin) (void)hipHostFree(c->h_pin);
  if (c->box) (void)hipHostFree(c->box);
  if (c->mb_pin) (void)hipHostFree(c->mb_pin);
  if (c->dfl_len) (void)hipHostFree(c->dfl_len);
  if (c->dfl_ev) (void)hipEventDestroy(c->dfl_ev);
  if (c->serial_ev) (void)hipEventDestroy(c->serial_ev);
  for (int i = 0; i < dctzhip_ctx::STAGE_WORKERS; i++) {
    if (c->stage[i]) (void)hipHostFree(c->stage[i]);
    if (c->stage_stream[i]) (void)hipStreamDestroy(c->stage_stream[i]);
  }
  for (int i = 0; i < 6; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  for (int q = 0; q < 2; q++) for (int i = 0; i < 5; i++) if (c->b_ev[q][i]) (void)hipEventDestroy(c->b_ev[q][i]);
  if (c->b_stream) { (void)hipStreamSynchronize(c->b_stream); (void)hipStreamDestroy(c->b_stream); }
  if (c->b_fork) (void)hipEventDestroy(c->b_fork);
  if (c->b_join) (void)hipEventDestroy(c->b_join);
  { void* bb[] = {c->b_ctl, c->b_guess, c->b_stats, c->b_remcnt, c->b_blob_dev};
    for (void* b : bb) if (b) (void)hipFree(b);
    for (int q = 0; q < 2; q++) for (int l = 0; l < 64; l++) if (c->rtab_cache[q][l]) (void)hipFree(c->rtab_cache[q][l]);
    if (c->b_blob) (void)hipHostFree(c->b_blob);
    if (c->b_res) (void)hipHostFree(c->b_res); }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

// NULL is the legacy default stream (what a caller that never created a stream works on), exactly like a
// NULL hipStream_t anywhere else in HIP; the context's private stream is selected with dctzhip_use_own_stream.
extern "C" int dctzhip_set_stream(dctzhip_ctx* c, void* s) {
  if (!c) return DCTZHIP_E_ARG;
  c->stream = (hipStream_t)s;
  c->memo.valid = false;                            // (the tables were written in the order of the stream that is left)
  return DCTZHIP_OK;
}
extern "C" int dctzhip_set_decode_memo(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->dec_memo = on != 0;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_use_own_stream(dctzhip_ctx* c) {
  if (!c) return DCTZHIP_E_ARG;
  c->memo.valid = false;
  c->stream = c->own_stream;
  return DCTZHIP_OK;
}
extern "C" void* dctzhip_get_stream(dctzhip_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int dctzhip_set_profiling(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->profiling = on ? 1 : 0;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_set_blocking(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->blocking = on != 0;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_set_speculation(dctzhip_ctx* c, int on, size_t min_elements) {
  if (!c) return DCTZHIP_E_ARG;
  c->speculate = on != 0;
  c->spec_cooldown = 0;
  if (!on) c->spec_mem.clear();
  if (min_elements) c->spec_min = min_elements;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_set_spec_memory(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->spec_memory = on != 0;
  c->spec_mem.clear();
  return DCTZHIP_OK;
}
// (tools) the name rocprofv3 lists the big kernel of the last call under -- every template argument -- so that bench.py can ask
// the committed traffic record for exactly the kernel it timed
template <typename T> static const char* tname() { return sizeof(T) == 8 ? "double" : "float"; }
static const char* bname(bool b) { return b ? "true" : "false"; }
#define SET_LAST(c, slot, ...) snprintf((c)->last_kernel[slot], sizeof((c)->last_kernel[slot]), __VA_ARGS__)
extern "C" int dctzhip_debug_last_kernel(dctzhip_ctx* c, int which, char* buf, size_t cap) {
  if (!c || !buf || cap == 0 || which < 0 || which > 5) return DCTZHIP_E_ARG;
  snprintf(buf, cap, "%s", c->last_kernel[which]);
  return DCTZHIP_OK;
}
// (tests and tools) counters of the context, and knobs that make a rare path run on purpose
extern "C" int dctzhip_debug_counter(dctzhip_ctx* c, int which, unsigned long long* value) {
  if (!c || !value) return DCTZHIP_E_ARG;
  switch (which) {
    case 0: *value = c->one_calls; break;
    case 1: *value = c->one_fallbacks; break;
    case 2: *value = (unsigned long long)c->one_cooldown; break;
    case 3: *value = c->eo_calls; break;
    case 4: *value = c->eo_direct_calls; break;
    case 5: *value = c->eo_lb_fallbacks; break;
    case 6: *value = c->spec_hits; break;
    case 7: *value = c->spec_misses; break;
    case 8: *value = c->b_spec_items; break;         // batch items that took their scaling factor from a sample
    case 9: *value = c->b_spec_misses; break;        // ... whose guess the true statistics refused (done again on their own)
    case 10: *value = c->rd_stepdowns; break;        // dctzhip_compress_psnr: measured misses that stepped down a point of the grid
    case 11: *value = c->box_grid; break;            // dctzhip_decompress_box / _box_nd / _coarse_box_nd, last call: workgroups of its kernel
    case 12: *value = c->box_tiles; break;           // ... candidate tiles (more than workgroups: the grid-stride loop ran)
    case 13: *value = c->mbox_items; break;          // dctzhip_decompress_boxes / _boxes_nd / _coarse_boxes_nd, last call of any: (box, hit tile) items in its list
    case 14: *value = c->mbox_grid; break;           // ... workgroups of its decode launch (fewer than items: they took several each)
    case 15: *value = c->mbox_bound; break;          // ... the host's bound B of the items, the list's capacity
    case 16: *value = c->memo_decodes; break;        // dctzhip_decompress calls launched on the last compress call's tile counts (the decode memo)
    case 17: *value = c->memo_redos; break;          // ... of them, found stale by the decoder and done again behind k_count_tiles
    case 18: *value = c->hist_hits; break;           // speculative compress calls that took their guess from the remembered statistics of the same input, verified
    case 19: *value = c->hist_misses; break;         // ... refused by the true statistics (done again, like a sampled miss)
    case 20: *value = c->variant; break;             // dctzhip_compress / _compress_nd, last call: fast_sf | fast_bw << 8 of the pass that stands
    default: return fail(c, DCTZHIP_E_ARG, "dctzhip_debug_counter: no counter %d", which);
  }
  return DCTZHIP_OK;
}
extern "C" int dctzhip_debug_knob(dctzhip_ctx* c, int key, int value) {
  if (!c) return DCTZHIP_E_ARG;
  switch (key) {
    case 0: c->one_withhold = value != 0; break;     // workgroup 0 of the one-launch kernels withholds its granule: a launch that gives up
    case 1: c->eo_lb_fail = value != 0; break;       // one tile's look-back of k_compress_eo reports that it gave up
    case 2: c->one_cooldown = value; break;
    case 3: c->rd_sse_div = value > 1 ? value : 1; break;   // every predicted SSE of dctzhip_rd_probe divided by value (step-down path)
    case 4: c->one_epoch = (unsigned)value; break;   // the tag of the last one-launch kernel (value's 32 bits: -3 is 2^32 - 3), to meet the wrap
    default: return fail(c, DCTZHIP_E_ARG, "dctzhip_debug_knob: no knob %d", key);
  }
  return DCTZHIP_OK;
}
extern "C" int dctzhip_set_split(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->eo = on != 0;
  c->eo_direct = on == 3;
  c->eo_direct_pause = 0;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_set_one_launch(dctzhip_ctx* c, int on) {
  if (!c) return DCTZHIP_E_ARG;
  c->one = on != 0;
  c->one_cooldown = 0;
  return DCTZHIP_OK;
}
// (development: the time stamps of the last one-launch kernel, 16 per workgroup; DCTZHIP_ONE_STAMPS=1 at context creation)
extern "C" int dctzhip_debug_one_stamps(dctzhip_ctx* c, unsigned long long* host, size_t nwg) {
  if (!c || !host || !c->one_dbg || nwg > (size_t)ONE_BOARD) return DCTZHIP_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, c->one_dbg, sizeof(unsigned long long) * 16 * nwg, hipMemcpyDeviceToHost));
  return DCTZHIP_OK;
}
extern "C" int dctzhip_last_timings(dctzhip_ctx* c, dctzhip_timings* t) {
  if (!c || !t) return DCTZHIP_E_ARG;
  if (!c->have_timings) return fail(c, DCTZHIP_E_ARG, "no timings recorded (enable profiling first)");
  *t = c->last;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_malloc(dctzhip_ctx* c, void** dptr, size_t bytes) {
  if (!c || !dptr) return DCTZHIP_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(dptr, bytes ? bytes : 16));
  return DCTZHIP_OK;
}
extern "C" int dctzhip_free(dctzhip_ctx* c, void* dptr) {
  if (!c) return DCTZHIP_E_ARG;
  if (dptr) HIPCHK(c, hipFree(dptr));
  return DCTZHIP_OK;
}
extern "C" int dctzhip_memcpy_h2d(dctzhip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return DCTZHIP_E_ARG;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}
// A large copy into PAGEABLE host memory: the runtime's own path stages it through one pinned buffer on one thread
// (1 GiB: 45 ms, and first-touch page faults of a fresh destination are taken by that thread too).  Here eight worker
// threads each move every eighth 16 MiB piece: D2H into the worker's pinned slot on its own stream, then memcpy into
// the destination -- transfers and host copies of different workers overlap (1 GiB: ~20 ms).
static int staged_d2h(dctzhip_ctx* c, void* dst, const void* src, size_t bytes) {
  constexpr int W = dctzhip_ctx::STAGE_WORKERS;
  constexpr size_t SLOT = dctzhip_ctx::STAGE_SLOT;
  for (int i = 0; i < W; i++) {
    if (!c->stage[i]) HIPCHK(c, hipHostMalloc(&c->stage[i], SLOT, hipHostMallocDefault));
    if (!c->stage_stream[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->stage_stream[i], hipStreamNonBlocking));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));            // what the copy reads has been produced on the context's stream
  // (pieces of a slot's size, or smaller ones when that keeps every worker busy: a 64 MiB copy -- one group of the pipelined
  // dctz_decompress -- is thirty-two pieces of 2 MiB, not four of 16)
  size_t PIECE = SLOT;
  if (bytes < (size_t)4 * W * SLOT) {                  // (four pieces per worker: one worker's host copy runs under another's transfer)
    PIECE = ((bytes + 4 * W - 1) / (4 * W) + 4095) & ~(size_t)4095;
    if (PIECE < ((size_t)1 << 20)) PIECE = (size_t)1 << 20;
    if (PIECE > SLOT) PIECE = SLOT;
  }
  const size_t pieces = (bytes + PIECE - 1) / PIECE;
  hipError_t err[W];
  std::vector<std::thread> th;
  for (int w = 0; w < W; w++) {
    err[w] = hipSuccess;
    th.emplace_back([=, &err]() {
      if (hipSetDevice(c->device) != hipSuccess) { err[w] = hipErrorInvalidDevice; return; }
      for (size_t k = (size_t)w; k < pieces; k += W) {
        const size_t off = k * PIECE, len = bytes - off < PIECE ? bytes - off : PIECE;
        hipError_t e = hipMemcpyAsync(c->stage[w], (const char*)src + off, len, hipMemcpyDeviceToHost, c->stage_stream[w]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stage_stream[w]);
        if (e != hipSuccess) { err[w] = e; return; }
        memcpy((char*)dst + off, c->stage[w], len);
      }
    });
  }
  for (auto& t : th) t.join();
  for (int w = 0; w < W; w++) if (err[w] != hipSuccess) return fail(c, DCTZHIP_E_HIP, "staged D2H copy failed: %s", hipGetErrorString(err[w]));
  return DCTZHIP_OK;
}

// ---- a D2H copy that FOLLOWS its producer ------------------------------------------------------------------------------
// dctz_decompress rebuilds a large array group by group (libdctz.c: decompress_pipelined); the copy of the reconstruction
// into the caller's (pageable) array is one continuous stream of pieces through the pinned slots above, started before the
// first group exists: a piece is moved as soon as the producer has announced its range (dctzhip_d2h_pipe_advance: an event
// on the context's stream behind the kernels that write it -- the workers' streams wait for it on the GPU, no host sync).
//   begin(dst, src, bytes)   starts the workers          advance(upto)   bytes [0, upto) of src are complete in stream order
//   end()                    waits for the last piece
namespace {
struct D2hPipe {
  std::vector<std::thread> th;
  std::atomic<size_t> upto{0};
  std::atomic<int> nev{0};
  struct Mark { size_t upto; hipEvent_t ev; };
  Mark marks[DCTZHIP_D2H_PIPE_MAX_MARKS];
  std::atomic<int> failed{0};
  std::atomic<int> stop{0};
  bool active = false;
};
D2hPipe g_pipe;
}
extern "C" int dctzhip_d2h_pipe_begin(dctzhip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c || !dst || !src || !bytes) return DCTZHIP_E_ARG;
  if (g_pipe.active) return fail(c, DCTZHIP_E_ARG, "a D2H pipe is already open");
  constexpr int W = dctzhip_ctx::STAGE_WORKERS;
  constexpr size_t SLOT = dctzhip_ctx::STAGE_SLOT;
  HIPCHK(c, hipSetDevice(c->device));
  for (int i = 0; i < W; i++) {
    if (!c->stage[i]) HIPCHK(c, hipHostMalloc(&c->stage[i], SLOT, hipHostMallocDefault));
    if (!c->stage_stream[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->stage_stream[i], hipStreamNonBlocking));
  }
  g_pipe.upto = 0; g_pipe.nev = 0; g_pipe.failed = 0; g_pipe.stop = 0; g_pipe.active = true;
  const size_t PIECE = (size_t)4 << 20;
  const size_t pieces = (bytes + PIECE - 1) / PIECE;
  for (int w = 0; w < W; w++) {
    g_pipe.th.emplace_back([=]() {
      if (hipSetDevice(c->device) != hipSuccess) { g_pipe.failed = 1; return; }
      int seen = 0;                                   // marks this worker has made its stream wait for
      for (size_t k = (size_t)w; k < pieces; k += W) {
        const size_t off = k * PIECE, len = bytes - off < PIECE ? bytes - off : PIECE;
        while (g_pipe.upto.load(std::memory_order_acquire) < off + len) {
          if (g_pipe.stop.load() || g_pipe.failed.load()) return;
          std::this_thread::yield();
        }
        // the youngest mark that covers the piece: the stream waits for its event (older marks are implied: one stream)
        const int n = g_pipe.nev.load(std::memory_order_acquire);
        int need = seen;
        while (need < n && g_pipe.marks[need].upto < off + len) need++;
        if (need < n && need >= seen) {
          if (hipStreamWaitEvent(c->stage_stream[w], g_pipe.marks[need].ev, 0) != hipSuccess) { g_pipe.failed = 1; return; }
          seen = need + 1;
        }
        hipError_t e = hipMemcpyAsync(c->stage[w], (const char*)src + off, len, hipMemcpyDeviceToHost, c->stage_stream[w]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stage_stream[w]);
        if (e != hipSuccess) { g_pipe.failed = 1; return; }
        memcpy((char*)dst + off, c->stage[w], len);
      }
    });
  }
  return DCTZHIP_OK;
}
extern "C" int dctzhip_d2h_pipe_advance(dctzhip_ctx* c, size_t upto) {
  if (!c || !g_pipe.active) return DCTZHIP_E_ARG;
  const int n = g_pipe.nev.load();
  if (n >= DCTZHIP_D2H_PIPE_MAX_MARKS) return fail(c, DCTZHIP_E_ARG, "too many marks in one D2H pipe");
  hipEvent_t ev;
  HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(ev, c->stream));
  g_pipe.marks[n].upto = upto; g_pipe.marks[n].ev = ev;
  g_pipe.nev.store(n + 1, std::memory_order_release);
  g_pipe.upto.store(upto, std::memory_order_release);
  return DCTZHIP_OK;
}
extern "C" int dctzhip_d2h_pipe_end(dctzhip_ctx* c, int abandon) {
  if (!c || !g_pipe.active) return DCTZHIP_E_ARG;
  if (abandon) g_pipe.stop = 1;
  for (auto& t : g_pipe.th) t.join();
  g_pipe.th.clear();
  for (int i = 0; i < g_pipe.nev.load(); i++) (void)hipEventDestroy(g_pipe.marks[i].ev);
  g_pipe.active = false;
  if (g_pipe.failed.load()) return fail(c, DCTZHIP_E_HIP, "pipelined D2H copy failed");
  return DCTZHIP_OK;
}

// ---- an H2D copy its CONSUMER follows ----------------------------------------------------------------------------------
// dctz_compress of a large array (libdctz.c: compress_pipelined) starts the kernels of a group of elements as soon as that
// group is on the device, while the rest of the caller's (pageable) array is still crossing PCIe.  One thread issues the
// groups in order on a stream of its own and records an event behind each.
//   begin(dst, src, bytes, group)   starts the thread
//   wait(upto)     the context's stream waits (on the GPU) for the group that ends at or behind `upto`; the host only
//                  waits until that copy has been ISSUED
//   landed(upto)   the host waits until bytes [0, upto) are on the device -- the source is no longer read (the in-place
//                  x /= sf of the caller's array follows the copy at this distance)
//   end(abandon)
namespace {
struct H2dPipe {
  std::thread th;
  std::atomic<int> issued{0};
  std::atomic<int> failed{0};
  std::atomic<int> stop{0};
  std::vector<hipEvent_t> ev;
  size_t group = 0, bytes = 0;
  hipStream_t st = nullptr;
  int device = -1;
  int waited = 0;                                     // events the context's stream already waits for
  bool active = false;
};
H2dPipe g_h2d;
}
extern "C" int dctzhip_h2d_pipe_begin(dctzhip_ctx* c, void* d_dst, const void* src, size_t bytes, size_t group_bytes) {
  if (!c || !d_dst || !src || !bytes || !group_bytes) return DCTZHIP_E_ARG;
  if (g_h2d.active) return fail(c, DCTZHIP_E_ARG, "an H2D pipe is already open");
  HIPCHK(c, hipSetDevice(c->device));
  if (g_h2d.st && g_h2d.device != c->device) { (void)hipStreamDestroy(g_h2d.st); g_h2d.st = nullptr; }
  if (!g_h2d.st) { HIPCHK(c, hipStreamCreateWithFlags(&g_h2d.st, hipStreamNonBlocking)); g_h2d.device = c->device; }
  const size_t ngroups = (bytes + group_bytes - 1) / group_bytes;
  if (ngroups > DCTZHIP_H2D_PIPE_MAX_GROUPS) return fail(c, DCTZHIP_E_ARG, "too many groups in one H2D pipe");
  g_h2d.ev.resize(ngroups);
  for (size_t i = 0; i < ngroups; i++) HIPCHK(c, hipEventCreateWithFlags(&g_h2d.ev[i], hipEventDisableTiming));
  g_h2d.issued = 0; g_h2d.failed = 0; g_h2d.stop = 0; g_h2d.waited = 0;
  g_h2d.group = group_bytes; g_h2d.bytes = bytes; g_h2d.active = true;
  const int device = c->device;
  g_h2d.th = std::thread([=]() {
    if (hipSetDevice(device) != hipSuccess) { g_h2d.failed = 1; return; }
    for (size_t g = 0; g < ngroups; g++) {
      if (g_h2d.stop.load()) return;
      const size_t off = g * group_bytes, len = bytes - off < group_bytes ? bytes - off : group_bytes;
      hipError_t e = hipMemcpyAsync((char*)d_dst + off, (const char*)src + off, len, hipMemcpyHostToDevice, g_h2d.st);
      if (e == hipSuccess) e = hipEventRecord(g_h2d.ev[g], g_h2d.st);
      if (e != hipSuccess) { g_h2d.failed = 1; return; }
      g_h2d.issued.store((int)g + 1, std::memory_order_release);
    }
  });
  return DCTZHIP_OK;
}
static int h2d_group_of(size_t upto) {                // index of the group that holds byte upto - 1
  if (upto > g_h2d.bytes) upto = g_h2d.bytes;
  return upto ? (int)((upto - 1) / g_h2d.group) : -1;
}
static int h2d_issued(dctzhip_ctx* c, int g) {
  while (g_h2d.issued.load(std::memory_order_acquire) <= g) {
    if (g_h2d.failed.load()) return fail(c, DCTZHIP_E_HIP, "pipelined H2D copy failed");
    std::this_thread::yield();
  }
  return DCTZHIP_OK;
}
extern "C" int dctzhip_h2d_pipe_wait(dctzhip_ctx* c, size_t upto) {
  if (!c || !g_h2d.active) return DCTZHIP_E_ARG;
  const int g = h2d_group_of(upto);
  if (g < 0 || g < g_h2d.waited) return DCTZHIP_OK;
  int rc = h2d_issued(c, g);
  if (rc) return rc;
  HIPCHK(c, hipStreamWaitEvent(c->stream, g_h2d.ev[g], 0));
  g_h2d.waited = g + 1;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_h2d_pipe_landed(dctzhip_ctx* c, size_t upto) {
  if (!c || !g_h2d.active) return DCTZHIP_E_ARG;
  const int g = h2d_group_of(upto);
  if (g < 0) return DCTZHIP_OK;
  int rc = h2d_issued(c, g);
  if (rc) return rc;
  HIPCHK(c, hipEventSynchronize(g_h2d.ev[g]));
  return DCTZHIP_OK;
}
extern "C" int dctzhip_h2d_pipe_end(dctzhip_ctx* c, int abandon) {
  if (!c || !g_h2d.active) return DCTZHIP_E_ARG;
  if (abandon) g_h2d.stop = 1;
  if (g_h2d.th.joinable()) g_h2d.th.join();
  hipError_t e = hipStreamSynchronize(g_h2d.st);
  for (auto& ev : g_h2d.ev) (void)hipEventDestroy(ev);
  g_h2d.ev.clear();
  g_h2d.active = false;
  if (g_h2d.failed.load() || e != hipSuccess) return fail(c, DCTZHIP_E_HIP, "pipelined H2D copy failed");
  return DCTZHIP_OK;
}

extern "C" int dctzhip_memcpy_d2h(dctzhip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return DCTZHIP_E_ARG;
  if (c->staged_d2h && bytes >= ((size_t)16 << 20)) {
    hipPointerAttribute_t at;
    const bool pageable = hipPointerGetAttributes(&at, dst) != hipSuccess || at.type == hipMemoryTypeUnregistered;
    (void)hipGetLastError();
    if (pageable) return staged_d2h(c, dst, src, bytes);
  }
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}
// A D2H copy beside the context's stream (the pipelined dctz_compress brings the compressed pieces of finished groups back on
// a thread of its own while the calling thread queues the next group's kernels): the caller vouches that the source is
// complete -- it has synchronised with its producer -- and that at most one thread makes such copies at a time.
extern "C" int dctzhip_memcpy_d2h_side(dctzhip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c || (bytes && (!dst || !src))) return DCTZHIP_E_ARG;
  if (!bytes) return DCTZHIP_OK;
  if (hipSetDevice(c->device) != hipSuccess) return DCTZHIP_E_HIP;     // (called from a thread of its own: libdctz's drainer)
  if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->side_stream) != hipSuccess) return DCTZHIP_E_HIP;
  if (hipStreamSynchronize(c->side_stream) != hipSuccess) return DCTZHIP_E_HIP;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_host_register(dctzhip_ctx* c, void* ptr, size_t bytes) {
  if (!c || !ptr || !bytes) return DCTZHIP_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return DCTZHIP_OK;
}
extern "C" int dctzhip_host_unregister(dctzhip_ctx* c, void* ptr) {
  if (!c || !ptr) return DCTZHIP_E_ARG;
  HIPCHK(c, hipHostUnregister(ptr));
  return DCTZHIP_OK;
}

template <typename P> static int regrow(dctzhip_ctx* c, P** ptr, size_t* cap, size_t need, size_t elem);
// ---------------------------------------------------------------- GPU entropy stage --
// the zlib tail of dctz_compress (dctz-comp-lib.c:620-732) on the device.  Every section becomes
// one zlib stream that inflate() reads (dctz-decomp-lib.c:244-322); the bytes differ from zlib's own (so do zlib's
// between versions), the inflated content is identical.
extern "C" size_t dctzhip_deflate_bound(size_t n) { return deflate_bound(n); }
extern "C" size_t dctzhip_deflate_chunk_bytes(void) { return deflate_chunk_bytes(); }

extern "C" int dctzhip_deflate_ex(dctzhip_ctx* c, int nsec, const void* const* d_src, const size_t* n, void* const* d_dst, const size_t* cap,
                                  size_t* out_len, uint32_t* const* chunk_sizes, const unsigned* flags) {
  if (!c || nsec < 0 || nsec > 8 || (nsec && (!d_src || !n || !d_dst || !cap || !out_len))) return fail(c, DCTZHIP_E_ARG, "dctzhip_deflate: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->dfl_len) {
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->dfl_len), 8 * sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->dfl_len_dev), c->dfl_len, 0));
  }
  size_t need = 0;
  for (int i = 0; i < nsec; i++) {
    if (n[i] && !d_src[i]) return fail(c, DCTZHIP_E_ARG, "dctzhip_deflate: section %d has no source", i);
    if (!d_dst[i] || cap[i] < deflate_bound(n[i])) return fail(c, DCTZHIP_E_ARG, "dctzhip_deflate: section %d needs %zu bytes of output (dctzhip_deflate_bound)", i, deflate_bound(n[i]));
    if ((n[i] + deflate_chunk_bytes() - 1) / deflate_chunk_bytes() > 0x7FFFFFFFull) return fail(c, DCTZHIP_E_ARG, "dctzhip_deflate: section %d is too large", i);
    need += (deflate_scratch_bytes(n[i]) + 255) & ~(size_t)255;
  }
  {
    char* b = (char*)c->dfl_buf;
    int rc = regrow(c, &b, &c->dfl_cap, need, 1);
    c->dfl_buf = b;
    if (rc) return rc;
  }
  // The sections run side by side: the first on the context's stream, the others on the staging streams behind an
  // event of the context's stream (the small sections -- DC, AC_exact -- then cost nothing beside bin_index: each of
  // the four kernels of a section is latency bound by itself).  Every section has its own scratch.
  constexpr int SIDE = dctzhip_ctx::STAGE_WORKERS;
  const bool side = c->dfl_side && nsec > 1;
  if (side) {
    for (int i = 0; i < SIDE && i < nsec - 1; i++)
      if (!c->stage_stream[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->stage_stream[i], hipStreamNonBlocking));
    if (!c->dfl_ev) HIPCHK(c, hipEventCreateWithFlags(&c->dfl_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->dfl_ev, c->stream));
  }
  size_t at = 0;
  for (int i = 0; i < nsec; i++) {
    c->dfl_len[i] = 0;
    hipStream_t st = c->stream;
    if (side && i > 0) { st = c->stage_stream[(i - 1) % SIDE]; HIPCHK(c, hipStreamWaitEvent(st, c->dfl_ev, 0)); }
    HIPCHK(c, launch_deflate(d_src[i], n[i], d_dst[i], (char*)c->dfl_buf + at, c->dfl_len_dev + i, chunk_sizes ? chunk_sizes[i] : nullptr,
                             flags && (flags[i] & DCTZHIP_DEFLATE_LITERALS), st));
    at += (deflate_scratch_bytes(n[i]) + 255) & ~(size_t)255;
  }
  if (side)
    for (int i = 0; i < SIDE && i < nsec - 1; i++) HIPCHK(c, hipStreamSynchronize(c->stage_stream[i]));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < nsec; i++) out_len[i] = (size_t)c->dfl_len[i];
  return DCTZHIP_OK;
}
extern "C" int dctzhip_deflate(dctzhip_ctx* c, int nsec, const void* const* d_src, const size_t* n, void* const* d_dst, const size_t* cap,
                               size_t* out_len, uint32_t* const* chunk_sizes) {
  return dctzhip_deflate_ex(c, nsec, d_src, n, d_dst, cap, out_len, chunk_sizes, nullptr);
}
extern "C" int dctzhip_sync(dctzhip_ctx* c) {
  if (!c) return DCTZHIP_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

// The launch constants of dctz_quant_host.h into a parameter block, or into a batch record, which holds them widened to double
template <typename P, typename T>
static void set_quant(P& p, const InvQuant<T>& q) { p.bin_width = q.bin_width; p.range_min = q.range_min; p.range_max = q.range_max; }
template <typename P, typename T>
static void set_quant(P& p, const FwdQuant<T>& q) { p.bin_width = q.bin_width; p.range_min = q.range_min; p.range_max = q.range_max; p.fast_bw = q.fast_bw; }

static size_t elem_size(int dtype) { return dtype == DCTZHIP_F64 ? 8 : 4; }

// Inflate of sections written by dctzhip_deflate, chunk by chunk on the device (dctz_deflate.hip: k_dfl_inflate).
extern "C" int dctzhip_inflate(dctzhip_ctx* c, int nsec, const void* const* d_z, const size_t* zlen, const uint32_t* const* chunk_sizes,
                               const size_t* raw, void* const* d_dst, int* ok) {
  if (!c || !ok || nsec < 0 || nsec > 8 || (nsec && (!d_z || !zlen || !chunk_sizes || !raw || !d_dst))) return fail(c, DCTZHIP_E_ARG, "dctzhip_inflate: bad arguments");
  *ok = 0;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t chunk = deflate_chunk_bytes();
  // per section in the scratch: offsets (nch + 1) u32 | adler 2 x u64 | status u32
  std::vector<std::vector<uint32_t>> offs((size_t)nsec);
  size_t need = 0;
  std::vector<size_t> base((size_t)nsec);
  for (int i = 0; i < nsec; i++) {
    const size_t nch = (raw[i] + chunk - 1) / chunk;
    if (zlen[i] < 8 || (nch && !chunk_sizes[i]) || !d_z[i] || (raw[i] && !d_dst[i])) return DCTZHIP_OK;      // not ours: *ok stays 0
    offs[i].resize(nch + 1);
    unsigned long long run = 0;
    for (size_t k = 0; k < nch; k++) { offs[i][k] = (uint32_t)run; run += chunk_sizes[i][k]; if (chunk_sizes[i][k] == 0 || chunk_sizes[i][k] > chunk + 5) return DCTZHIP_OK; }
    offs[i][nch] = (uint32_t)run;
    if (run + 8 != zlen[i]) return DCTZHIP_OK;             // the sizes must tile the stream
    base[i] = need;
    need += ((nch + 1) * 4 + 15) / 16 * 16 + 32;
  }
  {
    char* b = (char*)c->dfl_buf;
    int rc = regrow(c, &b, &c->dfl_cap, need, 1);
    c->dfl_buf = b;
    if (rc) return rc;
  }
  // sections side by side, like dctzhip_deflate: a lane's 16 KiB take as long whatever the size of the section
  constexpr int SIDE = dctzhip_ctx::STAGE_WORKERS;
  const bool side = c->dfl_side && nsec > 1;
  if (side) {
    for (int i = 0; i < SIDE && i < nsec - 1; i++)
      if (!c->stage_stream[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->stage_stream[i], hipStreamNonBlocking));
    if (!c->dfl_ev) HIPCHK(c, hipEventCreateWithFlags(&c->dfl_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->dfl_ev, c->stream));
  }
  for (int i = 0; i < nsec; i++) {
    const size_t nch = offs[i].size() - 1;
    char* p = (char*)c->dfl_buf + base[i];
    unsigned long long* adler = (unsigned long long*)(p + ((nch + 1) * 4 + 15) / 16 * 16);
    uint32_t* status = (uint32_t*)(adler + 2);
    hipStream_t st = c->stream;
    if (side && i > 0) { st = c->stage_stream[(i - 1) % SIDE]; HIPCHK(c, hipStreamWaitEvent(st, c->dfl_ev, 0)); }
    HIPCHK(c, hipMemcpyAsync(p, offs[i].data(), (nch + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(status, 0, 4, st));
    HIPCHK(c, launch_inflate(d_z[i], (const uint32_t*)p, nch, raw[i], d_dst[i], adler, status, st));
  }
  if (side)
    for (int i = 0; i < SIDE && i < nsec - 1; i++) HIPCHK(c, hipStreamSynchronize(c->stage_stream[i]));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int good = 1;
  for (int i = 0; i < nsec; i++) {
    const size_t nch = offs[i].size() - 1;
    char* p = (char*)c->dfl_buf + base[i] + ((nch + 1) * 4 + 15) / 16 * 16;
    struct { unsigned long long a[2]; uint32_t status; uint32_t pad; } r;
    unsigned char tail[4];
    HIPCHK(c, hipMemcpy(&r, p, sizeof(r), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tail, (const char*)d_z[i] + zlen[i] - 4, 4, hipMemcpyDeviceToHost));
    const uint32_t s1 = (uint32_t)((1 + r.a[0]) % 65521u), s2 = (uint32_t)((raw[i] % 65521u + r.a[1]) % 65521u);
    const uint32_t want = ((uint32_t)tail[0] << 24) | ((uint32_t)tail[1] << 16) | ((uint32_t)tail[2] << 8) | tail[3];
    if (r.status != 0 || ((s2 << 16) | s1) != want) good = 0;      // what inflate() checks at the end of a stream
  }
  *ok = good;
  return DCTZHIP_OK;
}

template <typename P>
static int regrow(dctzhip_ctx* c, P** ptr, size_t* cap, size_t need, size_t elem) {
  if (need <= *cap) return DCTZHIP_OK;
  if (*ptr) HIPCHK(c, hipFree(*ptr));
  *ptr = nullptr; *cap = 0;
  HIPCHK(c, hipMalloc(ptr, need * elem));
  *cap = need;
  return DCTZHIP_OK;
}

// compress = true: scratch of the compress stage (workgroup-local lists); else decode (per-tile counts only)
static int ensure_scratch(dctzhip_ctx* c, size_t n, int dtype, int mode, bool compress = true, size_t min_entries = 0) {
  const size_t ntiles = (n / 64 + TILE_BLKS - 1) / TILE_BLKS;
  size_t entries = (ntiles > (size_t)PART_SLOTS ? ntiles : (size_t)PART_SLOTS) + 2;   // lists (<= grid + 1) or tiles, + the total
  if (entries < min_entries) entries = min_entries;
  int rc;
  {
    size_t cap = c->tile_cap, cap2 = c->tile_cap;
    if ((rc = regrow(c, &c->tile_cnt, &cap, entries, sizeof(unsigned)))) return rc;
    if ((rc = regrow(c, &c->tile_pre, &cap2, entries, sizeof(unsigned)))) return rc;
    if ((rc = regrow(c, &c->wg_cnt, &c->tile_cap, entries, sizeof(unsigned)))) return rc;
  }
  if (!compress) return DCTZHIP_OK;
  c->memo.valid = false;                               // (every call that rewrites ttot / memo_start comes through here first)
  if (ntiles + 2 > c->qcnt_cap) {                      // one word per block / per tile
    if (c->qcnt) HIPCHK(c, hipFree(c->qcnt));
    if (c->ttot) HIPCHK(c, hipFree(c->ttot));
    if (c->memo_start) HIPCHK(c, hipFree(c->memo_start));
    c->qcnt = nullptr; c->ttot = nullptr; c->memo_start = nullptr; c->qcnt_cap = 0;
    HIPCHK(c, hipMalloc(&c->qcnt, (ntiles + 2) * TILE_BLKS * sizeof(unsigned)));
    HIPCHK(c, hipMalloc(&c->ttot, (ntiles + 2) * sizeof(unsigned)));
    HIPCHK(c, hipMalloc(&c->memo_start, (ntiles + 2) * sizeof(unsigned)));
    c->qcnt_cap = ntiles + 2;
  }
  const size_t slots = (ntiles + 1) * TILE_ELEMS;      // list of workgroup b at the slot of its first tile; the remainder block's behind them
  if (mode == DCTZHIP_QT) {
    size_t cap_b = c->qt_cap;
    char* qi = (char*)c->qt_item;
    if ((rc = regrow(c, &qi, &cap_b, slots * elem_size(dtype), 1))) return rc;
    c->qt_item = qi; c->qt_cap = cap_b;
    if ((rc = regrow(c, &c->qt_j, &c->qtj_cap, slots, 1))) return rc;
  } else {
    if ((rc = regrow(c, &c->ac_tmp, &c->ac_tmp_cap, slots, sizeof(float)))) return rc;
  }
  return DCTZHIP_OK;
}

extern "C" int dctzhip_reserve(dctzhip_ctx* c, size_t n, int dtype, int mode) {
  if (!c) return DCTZHIP_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return ensure_scratch(c, n, dtype, mode);
}

static int check_common(dctzhip_ctx* c, size_t n, int dtype, int mode) {
  if (!c) return DCTZHIP_E_ARG;
  if (dtype != DCTZHIP_F32 && dtype != DCTZHIP_F64) return fail(c, DCTZHIP_E_ARG, "dtype must be DCTZHIP_F32 or DCTZHIP_F64");
  if (mode != DCTZHIP_EC && mode != DCTZHIP_QT) return fail(c, DCTZHIP_E_ARG, "mode must be DCTZHIP_EC or DCTZHIP_QT");
  if (n == 0) return fail(c, DCTZHIP_E_ARG, "n == 0");
  if (n > (size_t)INT_MAX) return fail(c, DCTZHIP_E_ARG, "n exceeds INT_MAX (dctz.h:126: N is an int); shard the array");
  return DCTZHIP_OK;
}
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---- the buffers of one call against each other (include/dctz_hip.h, "Buffers of one call") ----
// Every buffer of a call is a byte range: READ (an input), IN_PLACE (an input that its own item divides by sf at the end:
// d_scaled == d_in) or OUT (bin_index, DC, the capacity of AC_exact, a separate scaled copy, the coefficient tap, a decode's
// output).  Any number of READ ranges may overlap each other and IN_PLACE ranges; everything else that overlaps is refused.
namespace {
enum { SPAN_READ = 0, SPAN_IN_PLACE = 1, SPAN_OUT = 2 };
struct Span { uintptr_t lo, hi; int kind, item; };
}
static void add_span(Span* v, size_t* m, const void* p, size_t bytes, int kind, int item) {
  if (p && bytes) v[(*m)++] = Span{(uintptr_t)p, (uintptr_t)p + bytes, kind, item};
}
// Sorted by start, a range overlaps an earlier one iff that one ends beyond its start: O(m log m).  shared (or null): set for
// every item whose IN_PLACE range another item reads -- its division has to wait for every read of the call.  In-place
// ranges are disjoint once the check passes, so the last one met is the only one that can cover a later start.
// unit (or null: "array", and the item of the later range is named): what an item is called; then a range that runs into an
// output names that output's item.
static int check_spans(dctzhip_ctx* c, Span* v, size_t m, const char* what, char* shared, const char* unit = nullptr) {
  std::sort(v, v + m, [](const Span& a, const Span& b) { return a.lo < b.lo; });
  uintptr_t end_any = 0, end_written = 0, end_out = 0, end_read = 0, ip_hi = 0;
  int ip_item = -1, out_item = -1;
  for (size_t i = 0; i < m; i++) {
    const Span& s = v[i];
    const uintptr_t end = s.kind == SPAN_OUT ? end_any : s.kind == SPAN_IN_PLACE ? end_written : end_out;
    if (end > s.lo && unit)
      return s.kind == SPAN_OUT ? fail(c, DCTZHIP_E_ARG, "%s: the output of %s %d overlaps another buffer of the call", what, unit, s.item)
                                : fail(c, DCTZHIP_E_ARG, "%s: the output of %s %d overlaps what the call reads", what, unit, out_item);
    if (end > s.lo)
      return fail(c, DCTZHIP_E_ARG, "%s: a buffer of array %d overlaps %s of the call", what, s.item,
                  s.kind == SPAN_READ ? "an output" : s.kind == SPAN_IN_PLACE ? "an output or another in-place range" : "another buffer");
    if (shared) {
      if (s.kind == SPAN_READ && ip_hi > s.lo && ip_item != s.item) shared[ip_item] = 1;
      if (s.kind == SPAN_IN_PLACE && end_read > s.lo) shared[s.item] = 1;
    }
    end_any = std::max(end_any, s.hi);
    if (s.kind != SPAN_READ) end_written = std::max(end_written, s.hi);
    if (s.kind == SPAN_OUT && s.hi > end_out) { end_out = s.hi; out_item = s.item; }
    if (s.kind == SPAN_READ) end_read = std::max(end_read, s.hi);
    if (s.kind == SPAN_IN_PLACE) { ip_hi = s.hi; ip_item = s.item; }
  }
  return DCTZHIP_OK;
}
// the ranges of one compress item; d_coef (single calls only) is n elements of the data type
static void compress_spans(Span* v, size_t* m, int item, const void* d_in, size_t n, int dtype, const void* d_bin, const void* d_dc,
                           const void* d_ac, const void* d_scaled, const void* d_coef) {
  const size_t es = dtype == DCTZHIP_F64 ? 8 : 4;
  const bool in_place = d_scaled && d_scaled == d_in;
  add_span(v, m, d_in, n * es, in_place ? SPAN_IN_PLACE : SPAN_READ, item);
  add_span(v, m, d_bin, n, SPAN_OUT, item);
  add_span(v, m, d_dc, (n + 63) / 64 * sizeof(float), SPAN_OUT, item);
  add_span(v, m, d_ac, n * sizeof(float), SPAN_OUT, item);
  if (!in_place) add_span(v, m, d_scaled, n * es, SPAN_OUT, item);
  add_span(v, m, d_coef, n * es, SPAN_OUT, item);
}
static void decompress_spans(Span* v, size_t* m, int item, const void* d_bin, const void* d_dc, const void* d_ac, uint32_t ac_count,
                             size_t n, int dtype, const void* d_out) {
  add_span(v, m, d_bin, n, SPAN_READ, item);
  add_span(v, m, d_dc, (n + 63) / 64 * sizeof(float), SPAN_READ, item);
  add_span(v, m, d_ac, (size_t)ac_count * sizeof(float), SPAN_READ, item);
  add_span(v, m, d_out, n * (dtype == DCTZHIP_F64 ? 8 : 4), SPAN_OUT, item);
}

// remainder-block tables -> device (cached per (l, dtype))
template <typename T>
static int upload_rtab(dctzhip_ctx* c, int l) {
  const int dt = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  if (c->rtab_l == l && c->rtab_dtype == dt) return DCTZHIP_OK;
  T* h = reinterpret_cast<T*>(c->h_pin + PIN_TAB);
  fill_rem_tab<T>(l, h);
  HIPCHK(c, hipMemcpyAsync(c->rtab, h, sizeof(T) * RTAB_SIZE, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // staging buffer is reused
  c->rtab_l = l; c->rtab_dtype = dt;
  return DCTZHIP_OK;
}

template <typename T> static const T* tab_of(dctzhip_ctx* c);
template <> const double* tab_of<double>(dctzhip_ctx* c) { return c->tab_f64; }
template <> const float* tab_of<float>(dctzhip_ctx* c) { return c->tab_f32; }

// Spin on a mailbox word until the kernels of this call have published `want`.  The stream is
// queried now and then so that a faulted launch ends the wait; after 10 s the call gives up.
static int wait_seq(dctzhip_ctx* c, volatile unsigned long long* word, unsigned long long want, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned long long spins = 1;; spins++) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return DCTZHIP_OK;
    __builtin_ia32_pause();
    if ((spins & 0xFFFF) == 0) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) {                        // everything ran: the word must be there now
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return DCTZHIP_OK;
        c->ctl_dirty = 1;
        return fail(c, DCTZHIP_E_INTERNAL, "%s: stream drained without publishing its result", what);
      }
      if (q != hipErrorNotReady) {
        c->ctl_dirty = 1;
        return fail(c, DCTZHIP_E_HIP, "%s: %s", what, hipGetErrorString(q));
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
        c->ctl_dirty = 1;
        return fail(c, DCTZHIP_E_INTERNAL, "%s: no result after 10 s", what);
      }
    }
  }
}

static int build_sf_tables(dctzhip_ctx* c) {
  const int kmin[2] = {-46, -324}, kmax[2] = {39, 309};          // decades of float / double, subnormals included
  for (int dt = 0; dt < 2; dt++) {
    const int nk = kmax[dt] - kmin[dt] + 1;
    double* thr = new double[nk];
    double* pw = new double[nk + 1];
    if (dt == DCTZHIP_F64) decade_tables<double>(kmin[dt], kmax[dt], thr, pw); else decade_tables<float>(kmin[dt], kmax[dt], thr, pw);
    // self-check against scaling_factor() on both sides of every boundary: a table that disagrees with the host's own
    // expression anywhere switches the device-side choice off (the host then chooses, as before)
    bool ok = true;
    for (int i = 0; i < nk && ok; i++) {
      const double probes[2] = {thr[i], dt == DCTZHIP_F64 ? nextafter(thr[i], INFINITY) : (double)nextafterf((float)thr[i], INFINITY)};
      for (double v : probes) {
        if (!(v > 0)) continue;                  // (v = inf is probed too: an array that holds an infinity gets sf = inf, util.c:29)
        int below = 0;
        for (int j = 0; j < nk; j++) below += thr[j] < v;
        const double want = scaling_factor(dt, v);
        if (!(pw[below] == want)) ok = false;
      }
    }
    if (!ok) c->dev_sf = 0;
    hipError_t e1 = hipMalloc(&c->sf_thr[dt], sizeof(double) * nk), e2 = hipMalloc(&c->sf_pw[dt], sizeof(double) * (nk + 1));
    if (e1 == hipSuccess && e2 == hipSuccess) {
      e1 = hipMemcpy(c->sf_thr[dt], thr, sizeof(double) * nk, hipMemcpyHostToDevice);
      e2 = hipMemcpy(c->sf_pw[dt], pw, sizeof(double) * (nk + 1), hipMemcpyHostToDevice);
    }
    delete[] thr; delete[] pw;
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(nullptr, DCTZHIP_E_HIP, "decade tables: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    c->sf_nk[dt] = nk;
  }
  HIPCHK(nullptr, hipMalloc(&c->sf_guess, sizeof(SfGuess)));
  return DCTZHIP_OK;
}

static int read_timings(dctzhip_ctx* c, int nev_main_start) {
  (void)nev_main_start;
  float a = 0, b = 0, d = 0, tot = 0;
  HIPCHK(c, hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
  HIPCHK(c, hipEventElapsedTime(&b, c->ev[2], c->ev[3]));
  HIPCHK(c, hipEventElapsedTime(&d, c->ev[3], c->ev[4]));
  tot = a + b + d;
  c->last.stats_ms = a; c->last.main_ms = b; c->last.tail_ms = d; c->last.total_ms = tot;
  c->have_timings = 1;
  return DCTZHIP_OK;
}

struct HostStats { double max_abs, min_abs, sum; };

// resident single-wave workgroups per CU of the two big kernels: what the runtime's occupancy calculator says for the
// instantiation (registers and LDS; k_compress: 8 for fp64, 12 for fp32 EC; k_decompress: 4 / 7), cached.
// A launch that takes the scaled variant of k_compress (takes_scaled) is sized by its UNSCALED twin's occupancy: the
// query passes scaled = false and the cache has no slot for it, although the scaled variants need a few registers more.
// Asking for the variant that runs would change grid sizes: a change of its own, to be measured before it is made.
template <typename T>
static int wg_per_cu(dctzhip_ctx* c, bool decode, int mode, bool stats = false, int geom = GEOM_1D) {
  if (c->wg_per_cu) return c->wg_per_cu;
  int& slot = c->occ[sizeof(T) == 8][decode ? 1 : 0][mode == DCTZHIP_QT][stats ? 1 : 0][geom];
  if (slot == 0) {
    int v = decode ? decompress_occupancy<T>(mode, geom) : compress_occupancy<T>(mode, stats, geom, false);
    if (v <= 0) {                                   // (no answer: the LDS bound alone)
      const size_t lds = decode ? decompress_lds_bytes<T>() : compress_lds_bytes<T>(mode);
      v = (int)((size_t)160 * 1024 / lds);
    }
    slot = v < 1 ? 1 : (v > WG_PER_CU_MAX ? WG_PER_CU_MAX : v);
  }
  return slot;
}

// *info of a compress call from what came back from the device (shared by the chain of kernels and the one-launch path)
static void fill_cinfo(dctzhip_cinfo* info, int dtype, int mode, double sf, const HostStats& st, size_t nm, unsigned cnt, unsigned nblk,
                       unsigned flags, const unsigned long long* qraw, unsigned long long q0bits) {
  memset(info, 0, sizeof(*info));
  info->sf = sf;
  // util.c:28 / :41: sum / N over the caller's array
  info->mean = (dtype == DCTZHIP_F64) ? st.sum / (double)(int)nm : (double)((float)st.sum / (float)(int)nm);
  info->max_abs = st.max_abs; info->min_abs = st.min_abs;
  info->cnt = cnt; info->nblk = nblk;
  info->flags = flags;
  if (mode == DCTZHIP_QT) {
    for (int j = 0; j < 64; j++) {
      double v;
      if (dtype == DCTZHIP_F64) { unsigned long long b = qraw[j]; memcpy(&v, &b, 8); }
      else { unsigned int b = (unsigned int)qraw[j]; float f; memcpy(&f, &b, 4); v = f; }
      info->qtable_raw[j] = v;
      info->qtable[j] = (j >= 1 && v < 1.0) ? 1.0 : v;          // :450-461
    }
    double q0;
    if (dtype == DCTZHIP_F64) { unsigned long long b = q0bits; memcpy(&q0, &b, 8); }
    else { unsigned int b = (unsigned int)q0bits; float f; memcpy(&f, &b, 4); q0 = f; }
    info->qtable[0] = info->qtable_raw[0] = q0;                 // :355-360
  }
}

// ---- one launch per call (dctz_kernels_one.hip) ----------------------------------------------------------------------
// Arrays whose tiles are all resident at once -- ONE_TW tiles per workgroup, as many workgroups as the chip holds -- go
// through ONE kernel per call; everything else, and any call for which that kernel reports that its workgroups were not
// all resident (ONE_ERR_TIMEOUT: the occupancy query is advisory, another process may share the GPU), takes the chain.
static constexpr int ONE_DECLINED = 1;               // (positive: not an error code) the caller runs the chain of kernels
template <typename T>
static unsigned one_capacity(dctzhip_ctx* c, bool decode, int mode, bool scaled) {
  int& slot = c->one_occ[sizeof(T) == 8][decode ? 1 : 0][mode == DCTZHIP_QT][scaled ? 1 : 0];
  if (slot == 0) {
    const int v = decode ? decompress_one_occupancy<T>(mode) : compress_one_occupancy<T>(mode, scaled);
    slot = v < 1 ? -1 : (v > 8 ? 8 : v);
    if (getenv("DCTZHIP_ONE_DEBUG")) fprintf(stderr, "[dctzhip] one-launch occupancy f64=%d decode=%d qt=%d scaled=%d: %d workgroups per CU\n", (int)(sizeof(T) == 8), (int)decode, (int)(mode == DCTZHIP_QT), (int)scaled, v);
  }
  return slot > 0 ? (unsigned)(slot * c->num_cu) : 0u;
}
// The tag of the next one-launch kernel's granules.  The board is never cleared between launches -- a granule of another
// launch carries another tag -- so when the 32-bit tag wraps, the granules of 2^32 launches ago would pass for this launch's
// wherever a workgroup index has not been written since: the board is cleared on the wrap, in stream order in front of the
// launch (as lb_desc is on the wrap of lb_epoch).  0 on failure (never a tag).
static unsigned one_next_epoch(dctzhip_ctx* c) {
  if (++c->one_epoch == 0u) {
    if (hipMemsetAsync(c->one_ga, 0, sizeof(unsigned long long) * ONE_BOARD, c->stream) != hipSuccess ||
        hipMemsetAsync(c->one_gb, 0, sizeof(unsigned long long) * ONE_BOARD, c->stream) != hipSuccess ||
        hipMemsetAsync(c->one_rec, 0, sizeof(double) * 3 * ONE_BOARD, c->stream) != hipSuccess) {
      c->one_epoch = 0xFFFFFFFFu;                      // (the next call wraps, and clears, again)
      (void)fail(c, DCTZHIP_E_HIP, "one-launch board: clearing it on the wrap of the epoch failed");
      return 0u;
    }
    c->one_epoch = 1u;
  }
  return c->one_epoch;
}
// a launch gave up (or never reported): back to a known state, and the chain for a while
static int one_gave_up(dctzhip_ctx* c) {
  c->one_fallbacks++;
  c->one_cooldown = ONE_COOLDOWN;
  HIPCHK(c, hipMemsetAsync(c->one_ctl, 0, sizeof(Ctl) * 3, c->stream));
  HIPCHK(c, hipMemsetAsync(c->one_qt, 0, sizeof(unsigned long long) * 2 * ONE_QT_WORDS, c->stream));
  return DCTZHIP_OK;
}

template <typename T>
static int compress_one(dctzhip_ctx* c, const T* d_in, size_t n, double eb, int mode, uint8_t* d_bin, float* d_dc, float* d_ac,
                        T* d_scaled, T* d_coef, dctzhip_cinfo* info) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  if (!c->one || !c->handoff || !c->dev_sf || c->sf_nk[dtype] <= 0 || c->sf_nk[dtype] > 64 * (dtype == DCTZHIP_F64 ? 10 : 2)) return ONE_DECLINED;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  const unsigned nwg = (ntiles + ONE_TW - 1) / ONE_TW + (rem ? 1u : 0u);
  if (nwg > (unsigned)ONE_BOARD || nwg > one_capacity<T>(c, false, mode, d_scaled != nullptr)) return ONE_DECLINED;
  // In place (the scaled copy over the input: what the reference does to its caller's array) the chain of kernels takes the
  // call: k_compress_one stores x / sf over a tile BEFORE the sweeps that can still give up, and a launch that gives up with
  // half of the caller's array divided cannot be run again (the chain scales in place on verified statistics only)
  if (d_scaled && (const void*)d_scaled == (const void*)d_in) return ONE_DECLINED;
  if (c->one_cooldown > 0) { c->one_cooldown--; return ONE_DECLINED; }
  hipStream_t s = c->stream;
  if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
  const unsigned epoch = one_next_epoch(c);
  if (!epoch) return DCTZHIP_E_HIP;
  OneFwd<T> a;
  memset(&a, 0, sizeof(a));
  FwdParams<T>& p = a.p;
  p.x = d_in; p.bin = d_bin; p.dc = d_dc; p.ac = d_ac; p.coef = d_coef; p.scaled = d_scaled;
  p.tab = tab_of<T>(c); p.rtab = reinterpret_cast<const T*>(c->rtab);
  const unsigned slot = c->one_cslot;                // (the tables of maxima alternate between QT calls: a call's hand-off zeroes the other one)
  if (mode == DCTZHIP_QT) c->one_cslot ^= 1u;
  p.ctl = c->one_ctl;
  p.nfull = nfull; p.ntiles = ntiles; p.last_is_full = rem ? 0u : 1u;
  p.sf = (T)1;
  set_quant(p, fwd_quant<T>(eb, c->fastdiv));
  c->pass_fast_bw = p.fast_bw;
  a.b.ga = c->one_ga; a.b.gb = c->one_gb; a.b.rec = c->one_rec; a.b.epoch = epoch; a.b.nwg = nwg; a.b.dbg = c->one_dbg;
  a.sft = {c->sf_thr[dtype], c->sf_pw[dtype], c->sf_nk[dtype], c->fastdiv, dtype};
  a.box = c->box_dev;
  const unsigned long long seq = ++c->seq;
  a.seq = seq;
  a.qt = c->one_qt + slot * ONE_QT_WORDS; a.qt_next = c->one_qt + (slot ^ 1u) * ONE_QT_WORDS; a.qt_stride = ONE_QT_STRIDE; a.qt_shards = ONE_QT_SHARDS;
  a.eb = eb; a.rem = (unsigned)rem; a.bad_guess = (unsigned)c->one_bad_guess | (c->one_withhold ? 16u : 0u);
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[0], s)); HIPCHK(c, hipEventRecord(c->ev[1], s)); HIPCHK(c, hipEventRecord(c->ev[2], s)); }
  launch_compress_one<T>(a, mode, d_scaled != nullptr, s);
  SET_LAST(c, 0, "k_compress_one<%s, %d, %s>", tname<T>(), mode, bname(d_scaled != nullptr));
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[3], s)); HIPCHK(c, hipEventRecord(c->ev[4], s)); }
  HIPCHK(c, hipGetLastError());
  c->one_calls++;
  HostBox* hb = c->box;
  int rc = wait_seq(c, &hb->seq_done, seq, "compress (one launch)");
  if (rc) { (void)one_gave_up(c); return rc; }
  if (hb->error == ONE_ERR_TIMEOUT) {
    // (nothing the caller owns is lost: a call whose scaled copy goes over its input never comes here)
    rc = one_gave_up(c);
    return rc ? rc : ONE_DECLINED;
  }
  if (hb->error) { (void)one_gave_up(c); return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", hb->error); }
  if (c->profiling) { HIPCHK(c, hipEventSynchronize(c->ev[4])); rc = read_timings(c, 2); if (rc) return rc; }
  // the scaling factor the device chose from its decade tables against the host's own expression on the true statistics
  const HostStats st = {hb->fstats[0], hb->fstats[1], hb->fstats[2]};
  const double sf = hb->sf_used;
  double true_sf;
  if (!device_sf_stands(dtype, st.max_abs, st.min_abs, sf, hb->fast_used, &true_sf)) {
    c->one = 0;                                     // (a table bug: never seen; the chain has the host in its loop)
    if (d_scaled && (const void*)d_scaled == (const void*)d_in)
      return fail(c, DCTZHIP_E_INTERNAL, "scaling factor %g chosen on the device differs from the host's %g after an in-place pass", sf, true_sf);
    rc = one_gave_up(c);
    return rc ? rc : ONE_DECLINED;
  }
  c->variant = hb->fast_used | c->pass_fast_bw << 8;
  if (info) fill_cinfo(info, dtype, mode, true_sf, st, n, hb->cnt_total, nfull + (rem ? 1u : 0u), DCTZHIP_INFO_STATS_FUSED | DCTZHIP_INFO_ONE_LAUNCH,
                       const_cast<const unsigned long long*>(hb->qraw), hb->q0);
  return DCTZHIP_OK;
}

template <typename T>
static int decompress_one(dctzhip_ctx* c, const uint8_t* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                          const void* qtable_host, size_t n, double eb, double sf, int mode, T* d_out) {
  if (!c->one || !c->handoff) return ONE_DECLINED;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  const unsigned nwg = (ntiles + ONE_TW - 1) / ONE_TW + (rem ? 1u : 0u);
  if (nwg > (unsigned)ONE_BOARD || nwg > one_capacity<T>(c, true, mode, false)) return ONE_DECLINED;
  if (c->one_cooldown > 0) { c->one_cooldown--; return ONE_DECLINED; }
  hipStream_t s = c->stream;
  if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
  const unsigned epoch = one_next_epoch(c);
  if (!epoch) return DCTZHIP_E_HIP;
  OneInv<T> a;
  memset(&a, 0, sizeof(a));
  InvParams<T>& p = a.p;
  p.bin = d_bin; p.dc = d_dc; p.ac = d_ac; p.out = d_out;
  p.tab = tab_of<T>(c); p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.ctl = c->one_ctl + 2;
  p.nfull = nfull; p.ntiles = ntiles; p.ac_count = ac_count;
  p.sf = (T)sf;
  set_quant(p, inv_quant<T>(eb));
  p.eb = eb;
  if (mode == DCTZHIP_QT) memcpy(a.qtab, qtable_host, sizeof(T) * 64);      // (the table rides in the kernel's arguments: no copy in front of the launch)
  a.b.ga = c->one_ga; a.b.gb = c->one_gb; a.b.rec = c->one_rec; a.b.epoch = epoch; a.b.nwg = nwg; a.b.dbg = c->one_dbg;
  a.box = c->box_dev;
  const unsigned long long seq = ++c->seq;
  a.seq = seq;
  a.rem = (unsigned)rem;
  a.withhold = c->one_withhold ? 1u : 0u;
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[0], s)); HIPCHK(c, hipEventRecord(c->ev[1], s)); HIPCHK(c, hipEventRecord(c->ev[2], s)); }
  launch_decompress_one<T>(a, mode, s);
  SET_LAST(c, 1, "k_decompress_one<%s, %d>", tname<T>(), mode);
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[3], s)); HIPCHK(c, hipEventRecord(c->ev[4], s)); }
  HIPCHK(c, hipGetLastError());
  c->one_calls++;
  int rc = wait_seq(c, &c->box->seq_done, seq, "decompress (one launch)");
  if (rc) { (void)one_gave_up(c); return rc; }
  const unsigned err = c->box->error;
  if (err == ONE_ERR_TIMEOUT) { rc = one_gave_up(c); return rc ? rc : ONE_DECLINED; }
  if (c->profiling) { HIPCHK(c, hipEventSynchronize(c->ev[4])); rc = read_timings(c, 2); if (rc) return rc; }
  if (err == 2) return fail(c, DCTZHIP_E_ARG, "bin_index flags more exact coefficients than ac_count provides");
  if (err) return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", err);
  return DCTZHIP_OK;
}

// One pass of the compress kernels for a given set of statistics.  `fused`: the
// statistics are a guess (from a sample); k_compress recomputes the true ones on
// the way and leaves them in stats_out for the caller to check.
template <typename T>
static int compress_pass(dctzhip_ctx* c, const T* d_in, size_t n, double eb, int mode, uint8_t* d_bin, float* d_dc,
                         float* d_ac, T* d_coef, const HostStats& st, bool fused, double* sf_out, T* sf_t_out,
                         unsigned* fast_sf_out, unsigned long long seq, int geom, bool device_sf = false,
                         const NdDirect* nd = nullptr, T* d_scaled = nullptr, bool* zeroed_other = nullptr) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  hipStream_t s = c->stream;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  if (zeroed_other) *zeroed_other = false;           // (set where this pass's k_compact_ac zeroes the context's other control block)
  const double sf = device_sf ? 1.0 : scaling_factor(dtype, st.max_abs);   // (device_sf: k_stats_final_sf has chosen it; read back after the call)
  *sf_out = sf;
  c->memo.valid = false; c->memo_pass = false;       // (ttot / memo_start are about to be rewritten)

  FwdParams<T> p;
  memset(&p, 0, sizeof(p));
  p.x = d_in; p.bin = d_bin; p.dc = d_dc; p.ac = d_ac; p.coef = d_coef;
  p.scaled = d_scaled;                               // (k_compress writes x / sf there itself: compress_impl)
  p.qt_item = reinterpret_cast<T*>(c->qt_item); p.qt_j = c->qt_j;
  p.qcnt = c->qcnt; p.ttot = c->ttot;
  p.ac_tmp = c->ac_tmp;
  p.tile_cnt = c->tile_cnt;
  p.tab = tab_of<T>(c); p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.ctl = c->ctl;
  p.guess = device_sf ? c->sf_guess : nullptr;       // (then p.sf / p.fast_sf below are placeholders)
  if (nd) p.nd = *nd; else memset(&p.nd, 0, sizeof(p.nd));
  p.stat_part = fused ? c->part : nullptr;
  p.nfull = nfull; p.ntiles = ntiles; p.last_is_full = rem ? 0u : 1u;
  p.sf = (T)sf;
  set_quant(p, fwd_quant<T>(eb, c->fastdiv));
  p.fast_sf = fast_sf_level(dtype, c->fastdiv, (double)p.sf, st.min_abs, st.max_abs, !device_sf);
  *sf_t_out = p.sf; *fast_sf_out = p.fast_sf;
  c->pass_fast_bw = p.fast_bw;
  if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }

  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[2], s));
  // flat fp64 blocks, no scaled copy asked of the kernel: the form with a block over two lanes, if selected
  bool eo = false;
  if constexpr (sizeof(T) == 8) eo = c->eo && geom == GEOM_1D && !nd && d_scaled == nullptr && ntiles != 0;
  // ... and, in EC mode, with AC_exact placed by the kernel itself (look-back over the tiles' counts: no lists, no k_compact_ac)
  bool direct = eo && mode == DCTZHIP_EC && c->eo_direct;
  if (direct && c->eo_direct_pause > 0) { c->eo_direct_pause--; direct = false; }
  if (direct) {
    if ((size_t)ntiles + 64 > c->lb_cap) {
      if (c->lb_desc) HIPCHK(c, hipFree(c->lb_desc));
      c->lb_desc = nullptr; c->lb_cap = 0;
      HIPCHK(c, hipMalloc(&c->lb_desc, ((size_t)ntiles + 64) * sizeof(unsigned long long)));
      HIPCHK(c, hipMemsetAsync(c->lb_desc, 0, ((size_t)ntiles + 64) * sizeof(unsigned long long), s));
      c->lb_cap = (size_t)ntiles + 64;
    }
    if (++c->lb_epoch >= (1u << 30)) {               // (tags of 2^30 calls ago would match again)
      HIPCHK(c, hipMemsetAsync(c->lb_desc, 0, c->lb_cap * sizeof(unsigned long long), s));
      c->lb_epoch = 1;
    }
    if (!c->lb_ticket) { HIPCHK(c, hipMalloc(&c->lb_ticket, 128 * sizeof(unsigned))); HIPCHK(c, hipMemsetAsync(c->lb_ticket, 0, 128 * sizeof(unsigned), s)); }
    p.direct = c->eo_lb_fail ? 2u : 1u; p.lb_desc = c->lb_desc; p.lb_ticket = c->lb_ticket; p.lb_epoch = c->lb_epoch;
  }
  unsigned cap;
  if (eo) {
    int& slot = c->eo_occ[mode == DCTZHIP_QT][(fused ? 1 : 0) + (direct ? 2 : 0)];
    if (slot == 0) { const int v = compress_eo_occupancy(mode, fused, direct); slot = v < 1 ? 1 : (v > 8 ? 8 : v); }
    cap = (unsigned)(c->num_cu * (c->wg_per_cu ? (c->wg_per_cu < slot ? c->wg_per_cu : slot) : slot));
  } else {
    cap = (unsigned)(c->num_cu * wg_per_cu<T>(c, false, mode, fused, geom));
  }
  if (c->grid_c > 0 && (unsigned)c->grid_c < cap) cap = (unsigned)c->grid_c;       // DCTZHIP_GRID_C (experiments)
  const int grid = (int)(cap < ntiles ? cap : ntiles);
  p.nlists_main = (unsigned)grid;
  // launch-time check of the grid against what it indexes -- list lengths (+ the remainder block's), fused statistics
  // partials, per-tile words: whatever chose the grid (occupancy query, DCTZHIP_GRID_C / DCTZHIP_WG_PER_CU, a part with
  // more CUs than the tables were sized for), a grid that does not fit is refused here, not found out by a fault
  if ((size_t)grid + 2 > c->tile_cap || (fused && grid + 1 > PART_SLOTS) || (size_t)ntiles + 2 > c->qcnt_cap)
    return fail(c, DCTZHIP_E_INTERNAL, "compress grid of %d workgroups over %u tiles exceeds the scratch tables (%zu list entries, %d partials, %zu tiles)",
                grid, ntiles, c->tile_cap, PART_SLOTS, c->qcnt_cap);
  if constexpr (sizeof(T) == 8) {
    if (eo) {
      launch_compress_eo(p, mode, fused, grid, s); c->eo_calls++; if (direct) c->eo_direct_calls++;
      SET_LAST(c, 0, "k_compress_eo<%d, %s, %s>", mode, bname(fused), bname(direct));
    }
  }
  if (ntiles && !eo) {
    launch_compress<T>(p, mode, fused, grid, geom, s);
    SET_LAST(c, 0, "k_compress<%s, %d, %s, %d, %d, %s>", tname<T>(), mode, bname(fused), Phases<T>::C, geom, bname(takes_scaled(p, geom)));
  }
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[3], s));
  if (rem) launch_compress_rem<T>(p, mode, rem, s);
  // stitch the workgroup-local lists into AC_exact[]
  const unsigned nlists = (unsigned)grid + (rem ? 1u : 0u);
  // (QT: the per-position maxima of :371-372 are gathered by k_compress / k_compress_rem themselves while their items go
  // out; round 2 needed a pass over the lists for fp64)
  // (k_compact_ac finds the place of every list itself: no scan kernel.)  With the mailbox its first workgroup hands
  // the call's results to the host as soon as the kernel starts -- all of them are in by then -- so the host is back in
  // the caller, queueing the next call's launches, while the lists are still being moved
  // (... and zeroes the context's other control block for a next call that has no statistics kernel in front)
  const bool zeroing = seq != 0 && !direct;
  if (zeroed_other) *zeroed_other = zeroing;
  Ctl* const other = c->ctl == c->ctl_pair ? c->ctl_pair + 1 : c->ctl_pair;
  const FinArgs fin = {c->ctl, c->part, fused ? (int)nlists : 0, seq ? c->box_dev : nullptr, seq, p.guess,
                       zeroing ? reinterpret_cast<unsigned*>(other) : nullptr, (unsigned)(sizeof(Ctl) / 4)};
  if (direct) {
    // every exact coefficient is at its place and Ctl::cnt_total is final: only the hand-off is left
    if (seq) launch_finish(c->ctl, c->part, fused ? (int)nlists : 0, c->box_dev, seq, s, p.guess, c->lb_ticket, 128u);
    else HIPCHK(c, hipMemsetAsync(c->lb_ticket, 0, 128 * sizeof(unsigned), s));
  } else {
    // (the decode memo: flat blocks through k_compress, which leaves ttot[] -- k_compress_eo does not)
    const bool memo = geom == GEOM_1D && !nd && !eo && ntiles != 0;
    launch_compact_ac<T>(p, mode, eb, nlists, (int)nlists, fin, s, memo ? c->memo_start : nullptr);
    c->memo_pass = memo;
  }
  if (!seq && fused) launch_stats_final(c->part, (int)nlists, c->stats_out, s);
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[4], s));
  HIPCHK(c, hipGetLastError());
  return DCTZHIP_OK;
}

template <typename T>
static int stats_impl(dctzhip_ctx* c, const T* d_in, size_t n, double* max_abs, double* min_abs, double* sum);

// geom != GEOM_1D, nd == NULL: d_in is the block-linear layout of a multi-dimensional array (n = nblk * 64) and the
// statistics partials of the ORIGINAL array (n_orig elements) are already in c->part[0 .. pre_parts) -- k_gather_nd.
// geom != GEOM_1D, nd != NULL: d_in is the array itself, read in place by k_compress (no padding: n = nblk * 64 = N).
template <typename T>
static int compress_impl(dctzhip_ctx* c, const T* d_in, size_t n, double eb, int mode, uint8_t* d_bin, float* d_dc,
                         float* d_ac, T* d_scaled, T* d_coef, dctzhip_cinfo* info, int geom = GEOM_1D, int pre_parts = 0,
                         size_t n_orig = 0, const NdDirect* nd = nullptr) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  hipStream_t s = c->stream;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  const unsigned nblk = nfull + (rem ? 1 : 0);
  double* hs = reinterpret_cast<double*>(c->h_pin + PIN_STATS);    // [0..2] first statistics, [4..6] fused ones
  Ctl* hc = reinterpret_cast<Ctl*>(c->h_pin + PIN_CTL);
  // arrays whose tiles are all resident at once: the whole call is one kernel (dctz_kernels_one.hip)
  if (geom == GEOM_1D && !nd && pre_parts == 0) {
    const int rc1 = compress_one<T>(c, d_in, n, eb, mode, d_bin, d_dc, d_ac, d_scaled, d_coef, info);
    if (rc1 != ONE_DECLINED) return rc1;
  }

  // Speculation: calc_data_stat needs the whole array before the first division, i.e. a second
  // read of the input.  Only the DECADE of max|x| matters (util.c:29), so guess it from a sample,
  // let k_compress compute the true statistics while it streams the data anyway, and check the
  // guess afterwards; a wrong guess costs one re-run with the true values.  (The scaled copy the
  // reference's in-place semantics ask for is written at the very end, with the verified sf.)
  constexpr size_t chunk = (size_t)SWG * Traits<T>::EPV;
  const bool pre = pre_parts > 0;                   // statistics partials already there (k_gather_nd)
  bool spec = !pre && c->speculate && ntiles && n >= c->spec_min && n >= 4 * chunk * c->spec_group;
  if (spec && c->spec_cooldown > 0) { c->spec_cooldown--; spec = false; }
  // In place (d_scaled == d_in: what the reference does to its caller's array) k_compress can write x / sf back as well --
  // every half-tile is in registers before it is overwritten -- but only on verified statistics: a speculative pass with
  // a wrong guess would have destroyed the input it has to be run on again.  Such a call takes the full statistics pass
  // (0.16 ms per GiB) and saves the 2 s bytes / element of k_scale (0.42 ms).
  const bool scale_in_place = d_scaled && (const void*)d_scaled == (const void*)d_in && geom == GEOM_1D && !nd && c->fuse_scaled && ntiles && !pre;
  if (scale_in_place) spec = false;
  // the scaling factor is chosen on the device (k_stats_final_sf: from the sample of a speculative call, else from the
  // full statistics) and the main launch follows without asking the host; the host verifies it when the call is over
  const bool dsf = c->handoff != 0 && c->dev_sf && c->sf_nk[dtype] > 0;

  // Host hand-off: mailbox + spin, or D2H copy + stream sync
  const bool box = c->handoff != 0;
  HostBox* hb = c->box;
  auto reset = [&]() -> int {
    if (!box || c->ctl_dirty) HIPCHK(c, hipMemsetAsync(c->ctl, 0, sizeof(Ctl), s));   // (else: k_stats_final zeroes it)
    c->ctl_dirty = 1;                               // until this call's hand-off has been seen
    return DCTZHIP_OK;
  };
  // A speculative call on an input whose last calls all verified with one scaling factor guesses from THEIR true
  // statistics (dctz_spec_memory.h): no sample, no launch in front of k_compress.  The control block, which a statistics
  // kernel would have zeroed, is then the context's other one -- zeroed by the last call's k_compact_ac -- or, where that
  // one is not known to be clean (first call, a failed call, a call that went another way), memset like any other.
  SpecMemory::Entry hist_e;
  bool hist = false;
  // (not for an input the library owns -- the filled copy of dctzhip_compress_masked: every masked array of one size would
  // share its key, a rotation of unrelated fields the caller cannot see; such calls sample and leave the table alone)
  const bool remember = c->spec_memory && (const void*)d_in != c->mask_filled;
  if (spec && remember) {
    if (const SpecMemory::Entry* e = c->spec_mem.predict(d_in, n, dtype)) { hist_e = *e; hist = true; }
  }
  if (hist && box && c->ctl_other_clean) {
    c->ctl = c->ctl == c->ctl_pair ? c->ctl_pair + 1 : c->ctl_pair;
    c->ctl_other_clean = 0;                         // (the block that is left: until this call's k_compact_ac has zeroed it)
    c->ctl_dirty = 1;
  } else {
    if (hist) c->ctl_dirty = 1;                     // (no k_stats_final in front)
    int rc = reset();
    if (rc) return rc;
  }

  // ---- calc_data_stat (util.c:12-44): the full pass, or the sample -------------
  unsigned long long seq = box ? ++c->seq : 0ull;
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[0], s));
  const SfTable tab = {c->sf_thr[dtype], c->sf_pw[dtype], c->sf_nk[dtype], c->fastdiv, dtype};
  if (hist) {
    // nothing to launch
  } else if (pre) {
    launch_stats_final(c->part, pre_parts, c->stats_out, s, box ? c->box_dev : nullptr, seq, box ? c->ctl : nullptr,
                       dsf ? &tab : nullptr, c->sf_guess);
  } else if (spec) {
    const size_t ngroups = n / chunk / c->spec_group;
    // (half the statistics grid: the sample kernel keeps four chunks per workgroup in flight, and the final reduction
    // has half as many partials to fetch: 16.8 -> 13.8 us for the pair on 1 GiB)
    const size_t scap = (size_t)(c->stats_grid > 1 ? c->stats_grid / 2 : 1);
    const int sgrid = (int)(ngroups < scap ? ngroups : scap);
    launch_stats_sample<T>(d_in, n, c->spec_group, c->part, sgrid, c->stats_out, s, box ? c->box_dev : nullptr, seq, box ? c->ctl : nullptr,
                           dsf ? &tab : nullptr, c->sf_guess);
  } else {
    const size_t nvec = n / Traits<T>::EPV;
    int sgrid = (int)((nvec + SWG * 4 - 1) / (SWG * 4));
    if (sgrid < 1) sgrid = 1;
    if (sgrid > c->stats_grid) sgrid = c->stats_grid;
    launch_stats<T>(d_in, n, c->part, sgrid, c->stats_out, s, box ? c->box_dev : nullptr, seq, box ? c->ctl : nullptr,
                    dsf ? &tab : nullptr, c->sf_guess);
  }
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[1], s));
  HostStats st = {0.0, 0.0, 0.0};
  if (hist) {
    st = {hist_e.max_abs, hist_e.min_abs, 0.0};      // the host's guess: sf and the FastDiv level follow from it in compress_pass
  } else if (dsf) {
    // nothing to wait for: the scaling factor is chosen on the device (k_stats_final_sf) and the main launch follows at
    // once; the choice comes back with the call's results and is verified below
  } else if (box) {
    int rc = wait_seq(c, &hb->seq_stats, seq, "statistics");
    if (rc) return rc;
    st = {hb->stats[0], hb->stats[1], hb->stats[2]};
  } else {
    HIPCHK(c, hipMemcpyAsync(hs, c->stats_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    st = {hs[0], hs[1], hs[2]};
  }

  double sf = 1.0;
  T sf_t = T(1);
  unsigned fast_sf = 0;
  unsigned flags = 0;
  const unsigned long long eo0 = c->eo_calls, eod0 = c->eo_direct_calls, eof0 = c->eo_lb_fallbacks;
  bool respin = false;                              // second pass of a call: the host's own statistics and scaling factor
  // The scaled copy (dctz-comp-lib.c:193-216) is written by k_compress itself when it goes to a buffer of its own and the
  // blocks are flat (DCTZHIP_FUSE_SCALED=0: always the separate pass); a pass with a wrong guess of sf is run again with
  // the right one and writes it again.  In place (d_scaled == d_in) the call has been taken off the speculative path
  // above; for multi-dimensional blocks x / sf stays a pass of its own behind the kernels.
  T* const scaled_by_kernel = (scale_in_place || (d_scaled && (const void*)d_scaled != (const void*)d_in && geom == GEOM_1D && !nd && c->fuse_scaled)) ? d_scaled : nullptr;
  // one pass of the kernels + the hand-off of its results into *hc / hs[4..6]
  bool lb_retry = false;
  auto run = [&](const HostStats& stats, bool fused) -> int {
    const bool dev = dsf && !respin && !hist;
    bool zeroed_other = false;                        // the pass that stands had its k_compact_ac zero the context's other control block
    int rc = compress_pass<T>(c, d_in, n, eb, mode, d_bin, d_dc, d_ac, d_coef, stats, fused, &sf, &sf_t, &fast_sf, seq, geom, dev, nd, scaled_by_kernel, &zeroed_other);
    if (rc) return rc;
    if (box) {
      rc = wait_seq(c, &hb->seq_done, seq, "compress");
      if (rc) return rc;
      c->ctl_dirty = 0;
      if (dev) { sf = hb->sf_used; sf_t = (T)sf; fast_sf = hb->fast_used; }
      hc->cnt_total = hb->cnt_total; hc->error = hb->error; hc->q0 = hb->q0;
      for (int j = 0; j < 64; j++) hc->qraw[j] = hb->qraw[j];
      hs[4] = hb->fstats[0]; hs[5] = hb->fstats[1]; hs[6] = hb->fstats[2];
      if (c->profiling) HIPCHK(c, hipEventSynchronize(c->ev[4]));
    } else {
      if (fused) HIPCHK(c, hipMemcpyAsync(hs + 4, c->stats_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(hc, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipStreamSynchronize(s));
    }
    if (hc->error == 5u && !lb_retry) {              // EO_ERR_LOOKBACK: a look-back of k_compress_eo gave up (a workgroup that held a chunk made no progress)
      lb_retry = true;                                // -> the same pass through the lists, and the lists for the next calls
      c->eo_lb_fallbacks++; c->eo_direct_pause = 64;
      c->ctl_dirty = 1;
      rc = reset();
      if (rc) return rc;
      if (box) seq = ++c->seq;
      rc = compress_pass<T>(c, d_in, n, eb, mode, d_bin, d_dc, d_ac, d_coef, stats, fused, &sf, &sf_t, &fast_sf, seq, geom, dev, nd, scaled_by_kernel, &zeroed_other);
      if (rc) return rc;
      if (box) {
        rc = wait_seq(c, &hb->seq_done, seq, "compress");
        if (rc) return rc;
        c->ctl_dirty = 0;
        if (dev) { sf = hb->sf_used; sf_t = (T)sf; fast_sf = hb->fast_used; }
        hc->cnt_total = hb->cnt_total; hc->error = hb->error; hc->q0 = hb->q0;
        for (int j = 0; j < 64; j++) hc->qraw[j] = hb->qraw[j];
        hs[4] = hb->fstats[0]; hs[5] = hb->fstats[1]; hs[6] = hb->fstats[2];
        if (c->profiling) HIPCHK(c, hipEventSynchronize(c->ev[4]));
      } else {
        if (fused) HIPCHK(c, hipMemcpyAsync(hs + 4, c->stats_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(hc, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
      }
    }
    if (hc->error) { c->ctl_dirty = 1; return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", hc->error); }
    if (box) c->ctl_other_clean = zeroed_other;       // (the zeros were fenced before the hand-off that has just been seen)
    if (c->profiling) { rc = read_timings(c, 2); if (rc) return rc; }
    return DCTZHIP_OK;
  };
  { int rc = run(st, spec); if (rc) return rc; }

  if (spec || dsf) {
    // what the kernels used against what the TRUE statistics ask for (the fused ones of a speculative call; else the
    // full pass's own, which the device has turned into sf by the host's tables: a mismatch there would be a table bug)
    const HostStats truth = spec ? HostStats{hs[4], hs[5], hs[6]} : HostStats{hb->stats[0], hb->stats[1], hb->stats[2]};
    double true_sf;
    st = truth;
    if (device_sf_stands(dtype, truth.max_abs, truth.min_abs, (double)sf_t, fast_sf, &true_sf)) {
      sf = true_sf;
      if (spec) {
        flags |= DCTZHIP_INFO_STATS_FUSED; c->spec_hits++;
        if (hist) c->hist_hits++;
        if (remember) c->spec_mem.verified(d_in, n, dtype, truth.max_abs, truth.min_abs, true_sf);
      }
    } else {                                        // wrong guess: everything again with the true statistics
      if (scale_in_place)                           // (cannot happen: the device chose sf from the full statistics by the host's own tables)
        return fail(c, DCTZHIP_E_INTERNAL, "scaling factor %g chosen on the device differs from the host's %g after an in-place pass", (double)sf_t, true_sf);
      if (spec) {
        c->spec_misses++; c->spec_cooldown = SPEC_COOLDOWN;
        if (hist) c->hist_misses++;
        if (remember) c->spec_mem.missed(d_in, n, dtype, hist);
      }
      respin = true;
      flags |= DCTZHIP_INFO_RESPUN;
      c->ctl_dirty = 1;                             // the first pass left its QT maxima behind
      int rc = reset();
      if (rc) return rc;
      if (box) seq = ++c->seq;
      rc = run(st, false);
      if (rc) return rc;
    }
  }
  // The fused sum is 8 sf times the sum of the blocks' DCs.  A non-finite x[0] -- which util.c:22 never adds -- makes block
  // 0's DC and with it that whole sum NaN where the reference's is finite, so a fused sum that is not finite is taken again
  // by the plain pass, which leaves x[0] out (one more read, for arrays that hold a NaN or an infinity only).
  if (spec && !std::isfinite(st.sum)) {
    double mx2 = 0.0, mn2 = 0.0, sum2 = 0.0;
    int rc = stats_impl<T>(c, d_in, n, &mx2, &mn2, &sum2);
    if (rc) return rc;
    st.sum = sum2;
  }
  // dctz-comp-lib.c:193-216: the reference divides the caller's array by sf in place; here on request, into
  // d_scaled (which may be d_in itself), once sf is final
  if (d_scaled && !scaled_by_kernel) {
    if (sf_t != (T)1.0) launch_scale<T>(d_in, d_scaled, n, sf_t, c->num_cu * 8, s);
    else if ((const void*)d_scaled != (const void*)d_in) HIPCHK(c, hipMemcpyAsync(d_scaled, d_in, n * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipGetLastError());
  }

  c->variant = fast_sf | c->pass_fast_bw << 8;        // (fast_sf: what the device reported where it chose sf itself)
  if (c->eo_calls > eo0) flags |= DCTZHIP_INFO_SPLIT;
  if (c->eo_lb_fallbacks > eof0) flags |= DCTZHIP_INFO_LB_FALLBACK;
  else if (c->eo_direct_calls > eod0) flags |= DCTZHIP_INFO_SINGLE_PASS;
  if (info) fill_cinfo(info, dtype, mode, sf, st, n_orig ? n_orig : n, hc->cnt_total, nblk, flags, hc->qraw, hc->q0);
  // the decode memo: the tables of the pass that stands (after a respin: the second one's) describe these streams
  if (c->memo_pass && geom == GEOM_1D && !nd && pre_parts == 0) {
    c->memo.bin = d_bin; c->memo.dc = d_dc; c->memo.ac = d_ac; c->memo.n = n; c->memo.dtype = dtype; c->memo.mode = mode;
    c->memo.cnt_total = hc->cnt_total; c->memo.stream = s;
    c->memo.valid = true;
  }
  return DCTZHIP_OK;
}

template <typename T>
static int stats_impl(dctzhip_ctx* c, const T* d_in, size_t n, double* max_abs, double* min_abs, double* sum) {
  hipStream_t s = c->stream;
  const size_t nvec = n / Traits<T>::EPV;
  int sgrid = (int)((nvec + SWG * 4 - 1) / (SWG * 4));
  if (sgrid < 1) sgrid = 1;
  if (sgrid > c->stats_grid) sgrid = c->stats_grid;
  launch_stats<T>(d_in, n, c->part, sgrid, c->stats_out, s);
  double* hs = reinterpret_cast<double*>(c->h_pin + PIN_STATS);
  HIPCHK(c, hipMemcpyAsync(hs, c->stats_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  *max_abs = hs[0]; *min_abs = hs[1]; *sum = hs[2];
  return DCTZHIP_OK;
}

extern "C" int dctzhip_stats(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, dctzhip_cinfo* info) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_in || !info || !aligned16(d_in)) return fail(c, DCTZHIP_E_ARG, "bad buffer");
  HIPCHK(c, hipSetDevice(c->device));
  double mx, mn, sum;
  rc = (dtype == DCTZHIP_F64) ? stats_impl<double>(c, (const double*)d_in, n, &mx, &mn, &sum)
                              : stats_impl<float>(c, (const float*)d_in, n, &mx, &mn, &sum);
  if (rc) return rc;
  memset(info, 0, sizeof(*info));
  info->max_abs = mx; info->min_abs = mn;
  info->sf = scaling_factor(dtype, mx);
  info->mean = (dtype == DCTZHIP_F64) ? sum / (double)(int)n : (double)((float)sum / (float)(int)n);
  info->nblk = (uint32_t)((n + 63) / 64);
  return DCTZHIP_OK;
}

extern "C" int dctzhip_serial_mean_begin(dctzhip_ctx* c, const void* d_in, size_t n, int dtype) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_in) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  HIPCHK(c, hipSetDevice(c->device));
  // the input may still be in the making on the context's stream: the side stream reads behind what is queued there now
  if (!c->serial_ev) HIPCHK(c, hipEventCreateWithFlags(&c->serial_ev, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(c->serial_ev, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->side_stream, c->serial_ev, 0));
  if (dtype == DCTZHIP_F64) launch_serial_sum<double>((const double*)d_in, n, c->serial_out, c->side_stream);
  else launch_serial_sum<float>((const float*)d_in, n, c->serial_out, c->side_stream);
  HIPCHK(c, hipGetLastError());
  c->serial_n = n; c->serial_dtype = dtype;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_serial_mean_end(dctzhip_ctx* c, double* mean) {
  if (!c || !mean) return DCTZHIP_E_ARG;
  if (c->serial_dtype < 0) return fail(c, DCTZHIP_E_ARG, "dctzhip_serial_mean_begin was not called");
  double sum = 0.0;
  HIPCHK(c, hipMemcpyAsync(&sum, c->serial_out, sizeof(double), hipMemcpyDeviceToHost, c->side_stream));
  HIPCHK(c, hipStreamSynchronize(c->side_stream));
  // util.c:28 / :41 -- sum / N in the data type (N is an int)
  *mean = (c->serial_dtype == DCTZHIP_F64) ? sum / (double)(int)c->serial_n
                                           : (double)((float)sum / (float)(int)c->serial_n);
  c->serial_dtype = -1;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_debug_divide(dctzhip_ctx* c, const void* d_x, size_t n, int dtype, double divisor,
                                    void* d_fast, void* d_ref) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_x || !d_fast || !d_ref) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  HIPCHK(c, hipSetDevice(c->device));
  if (dtype == DCTZHIP_F64)
    launch_debug_divide<double>((const double*)d_x, n, divisor, (int)divisor_in_window(dtype, divisor), (double*)d_fast,
                                (double*)d_ref, c->stream);
  else
    launch_debug_divide<float>((const float*)d_x, n, (float)divisor, (int)divisor_in_window(dtype, (double)(float)divisor),
                               (float*)d_fast, (float*)d_ref, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

extern "C" int dctzhip_scale_inplace(dctzhip_ctx* c, void* d_x, size_t n, int dtype, double sf) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_x || !aligned16(d_x)) return fail(c, DCTZHIP_E_ARG, "bad buffer");
  HIPCHK(c, hipSetDevice(c->device));
  if (sf == 1.0) return DCTZHIP_OK;                 // dctz-comp-lib.c:193 / :208
  if (dtype == DCTZHIP_F64) launch_scale<double>((const double*)d_x, (double*)d_x, n, sf, c->num_cu * 8, c->stream);
  else launch_scale<float>((const float*)d_x, (float*)d_x, n, (float)sf, c->num_cu * 8, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

extern "C" int dctzhip_compress(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, double eb, int mode,
                                void* d_bin, float* d_dc, float* d_ac, void* d_scaled, void* d_coef,
                                dctzhip_cinfo* info) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  if (!d_in || !d_bin || !d_dc || !d_ac) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_in) || !aligned16(d_bin) || !aligned16(d_dc) || !aligned16(d_ac) ||
      (d_scaled && !aligned16(d_scaled)) || (d_coef && !aligned16(d_coef)))
    return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  if (eb < 1E-6) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  {
    Span sp[6];
    size_t m = 0;
    compress_spans(sp, &m, 0, d_in, n, dtype, d_bin, d_dc, d_ac, d_scaled, d_coef);
    rc = check_spans(c, sp, m, "dctzhip_compress", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_scratch(c, n, dtype, mode);
  if (rc) return rc;
  rc = (dtype == DCTZHIP_F64)
           ? compress_impl<double>(c, (const double*)d_in, n, eb, mode, (uint8_t*)d_bin, d_dc, d_ac, (double*)d_scaled, (double*)d_coef, info)
           : compress_impl<float>(c, (const float*)d_in, n, eb, mode, (uint8_t*)d_bin, d_dc, d_ac, (float*)d_scaled, (float*)d_coef, info);
  if (rc == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

// ---- a PART of an array whose statistics the caller already has ---------------------------------------------------------
// The streams of elements [lo, lo + n) of an array are the same whether the array is compressed in one call or part by
// part (blocks are independent, AC_exact is block-major), provided every part is scaled by the ARRAY's scaling factor
// (util.c:29) -- which is all that couples them.  dctz_compress of a large host array (libdctz.c: compress_pipelined) takes
// max|x| / min|x| of the whole array on host threads while the first parts cross PCIe and then runs the parts one by one,
// each as soon as it has landed.  EC only (QT's table is a property of the whole array, dctz-comp-lib.c:435-476).
// part_stats: max|x|, min|x| of the part and the sum of its elements FROM THE SECOND ON (util.c:22 starts at i = 1: the
// caller adds the first one where the part is not the array's first).
template <typename T>
static int compress_part_impl(dctzhip_ctx* c, const T* d_in, size_t n, double eb, const HostStats& st, uint8_t* d_bin, float* d_dc,
                              float* d_ac, uint32_t* cnt, double* part_stats, double* sf_out) {
  hipStream_t s = c->stream;
  double* hs = reinterpret_cast<double*>(c->h_pin + PIN_STATS);
  Ctl* hc = reinterpret_cast<Ctl*>(c->h_pin + PIN_CTL);
  const bool box = c->handoff != 0;
  HostBox* hb = c->box;
  HIPCHK(c, hipMemsetAsync(c->ctl, 0, sizeof(Ctl), s));      // (no statistics kernel in front that would do it)
  c->ctl_dirty = 1;
  const unsigned long long seq = box ? ++c->seq : 0ull;
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[0], s)); HIPCHK(c, hipEventRecord(c->ev[1], s)); }
  double sf = 1.0;
  T sf_t = T(1);
  unsigned fast_sf = 0;
  int rc = compress_pass<T>(c, d_in, n, eb, DCTZHIP_EC, d_bin, d_dc, d_ac, (T*)nullptr, st, true, &sf, &sf_t, &fast_sf, seq, GEOM_1D);
  if (rc) return rc;
  if (box) {
    rc = wait_seq(c, &hb->seq_done, seq, "compress (part)");
    if (rc) return rc;
    c->ctl_dirty = 0;
    hc->cnt_total = hb->cnt_total; hc->error = hb->error;
    hs[4] = hb->fstats[0]; hs[5] = hb->fstats[1]; hs[6] = hb->fstats[2];
    if (c->profiling) HIPCHK(c, hipEventSynchronize(c->ev[4]));
  } else {
    HIPCHK(c, hipMemcpyAsync(hs + 4, c->stats_out, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(hc, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  if (hc->error) { c->ctl_dirty = 1; return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", hc->error); }
  if (c->profiling) { rc = read_timings(c, 2); if (rc) return rc; }
  // the part's own extremes must lie inside the array's (else the caller's statistics are not this array's)
  if (hs[4] > st.max_abs || hs[5] < st.min_abs)
    return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_part: the part's max|x| %g / min|x| %g lie outside the statistics given (%g / %g)", hs[4], hs[5], st.max_abs, st.min_abs);
  *cnt = hc->cnt_total;
  if (part_stats) { part_stats[0] = hs[4]; part_stats[1] = hs[5]; part_stats[2] = hs[6]; }
  if (sf_out) *sf_out = sf;
  return DCTZHIP_OK;
}
extern "C" int dctzhip_compress_part(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, double eb, double max_abs, double min_abs,
                                     void* d_bin, float* d_dc, float* d_ac, uint32_t* cnt, double* part_stats, double* sf) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_in || !d_bin || !d_dc || !d_ac || !cnt) return fail(c, DCTZHIP_E_ARG, "null buffer");
  // (a part that starts at block b has its DC at d_dc + b: dword stores through a descriptor, like AC_exact's)
  if (!aligned16(d_in) || !aligned16(d_bin) || ((uintptr_t)d_dc & 3u) || ((uintptr_t)d_ac & 3u))
    return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned (DC, AC_exact: 4)");
  if (eb < 1E-6) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  // (max|x| = 0 with min|x| = the largest finite value is what the statistics say of an array that holds nothing but NaNs)
  const bool nothing_ordered = max_abs == 0.0 && min_abs == (dtype == DCTZHIP_F64 ? 1.79769313486231570815e308 : (double)3.40282346638528859812e38f);
  if (!nothing_ordered && (!(max_abs >= min_abs) || !(min_abs >= 0.0)))
    return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_part: statistics are not a max|x| >= min|x| >= 0 pair");
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_scratch(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  const HostStats st = {max_abs, min_abs, 0.0};
  rc = (dtype == DCTZHIP_F64)
           ? compress_part_impl<double>(c, (const double*)d_in, n, eb, st, (uint8_t*)d_bin, d_dc, d_ac, cnt, part_stats, sf)
           : compress_part_impl<float>(c, (const float*)d_in, n, eb, st, (uint8_t*)d_bin, d_dc, d_ac, cnt, part_stats, sf);
  if (rc == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

template <typename T>
static int decompress_impl(dctzhip_ctx* c, const uint8_t* d_bin, const float* d_dc, const float* d_ac,
                           uint32_t ac_count, const void* qtable_host, size_t n, double eb, double sf, int mode,
                           T* d_out, int geom = GEOM_1D, const NdDirect* nd = nullptr) {
  hipStream_t s = c->stream;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  const bool box = c->handoff != 0;                 // mailbox + spin instead of D2H copy + stream sync
  if (geom == GEOM_1D && !nd) {                     // arrays whose tiles are all resident at once: one kernel
    const int rc1 = decompress_one<T>(c, d_bin, d_dc, d_ac, ac_count, qtable_host, n, eb, sf, mode, d_out);
    if (rc1 != ONE_DECLINED) return rc1;
  }
  if (!box || c->ctl_dirty) HIPCHK(c, hipMemsetAsync(c->ctl, 0, sizeof(Ctl), s));      // (a good call leaves `error` at zero)
  c->ctl_dirty = 1;
  if (mode == DCTZHIP_QT && !ntiles) {              // (with tiles the table rides in k_count_tiles' arguments, below)
    // staged through pinned memory that the NEXT call may rewrite: safe because every call ends with a host
    // wait on this stream (mailbox or stream sync) before it returns
    T* hq = reinterpret_cast<T*>(c->h_pin + PIN_TAB + sizeof(double) * RTAB_SIZE);
    memcpy(hq, qtable_host, sizeof(T) * 64);
    HIPCHK(c, hipMemcpyAsync(c->qtab, hq, sizeof(T) * 64, hipMemcpyHostToDevice, s));
  }
  if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }

  InvParams<T> p;
  p.bin = d_bin; p.dc = d_dc; p.ac = d_ac; p.out = d_out;
  p.tab = tab_of<T>(c); p.rtab = reinterpret_cast<const T*>(c->rtab); p.qtab = reinterpret_cast<const T*>(c->qtab);
  p.ctl = c->ctl;
  p.tile_cnt = c->tile_cnt; p.wg_cnt = c->wg_cnt; p.tile_pre = nullptr;
  if (nd) p.nd = *nd; else memset(&p.nd, 0, sizeof(p.nd));
  p.nfull = nfull; p.ntiles = ntiles; p.ac_count = ac_count;
  p.sf = (T)sf;
  set_quant(p, inv_quant<T>(eb));
  p.eb = eb;
  const bool scale = (p.sf != (T)1.0);            // :496 / :505

  const unsigned cap = (unsigned)(c->num_cu * wg_per_cu<T>(c, true, mode, false, geom));
  const int grid = (int)(cap < ntiles ? cap : ntiles);
  p.nwg = (unsigned)grid;
  // tile-interleaved workgroups (k_decompress_il: the grid writes one contiguous window of the output at a time) for one
  // array of flat blocks whose workgroups take at most 64 tiles each
  if (c->dec_il && (c->dec_il == 2 || (sizeof(T) == 8 && mode == DCTZHIP_EC)) && geom == GEOM_1D && !nd && ntiles && (size_t)ntiles <= (size_t)64 * (size_t)grid && grid <= 4096)
    p.tile_pre = c->tile_pre;                       // (fp64 EC: the one combination it measured faster for, launch_decompress)
  // The decode memo: these are the streams the context's last compress call wrote, and its per-tile tables still stand ->
  // no pass over bin_index in front of the decoder, which checks the tables against the flags it reads (k_decompress_il,
  // MEMO) and reports a stale memo instead of a result; then the same call goes through k_count_tiles, below.
  const dctzhip_ctx::DecodeMemo& mm = c->memo;
  const bool memo = c->dec_memo && mm.valid && sizeof(T) == 8 && mode == DCTZHIP_EC && box && !rem && takes_interleaved(p, geom) &&
                    mm.bin == (const void*)d_bin && mm.dc == (const void*)d_dc && mm.ac == (const void*)d_ac && mm.n == n &&
                    mm.dtype == (sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32) && mm.mode == mode && mm.cnt_total == ac_count && mm.stream == s;
  if (memo) { p.tile_pre = c->memo_start; p.tile_cnt = c->ttot; }
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[0], s));
  // counts of "stored exactly" flags per tile and per workgroup of k_decompress: where every piece of AC_exact starts
  if (ntiles && !memo) launch_count_tiles(d_bin, nfull, ntiles, p.nwg, c->tile_cnt, c->wg_cnt, s, mode == DCTZHIP_QT ? qtable_host : nullptr, sizeof(T) * 64, c->qtab,
                                 const_cast<unsigned*>(p.tile_pre));
  if (c->profiling) { HIPCHK(c, hipEventRecord(c->ev[1], s)); HIPCHK(c, hipEventRecord(c->ev[2], s)); }
  const unsigned long long seq = box ? ++c->seq : 0ull;
  // With the mailbox and no remainder block, the first workgroup of k_decompress tells the host at once whether the
  // stream under-runs the caller's AC_exact (the counts are all in): the host is back in the caller while the
  // reconstruction is being written -- complete in stream order, like any launch.  Otherwise k_finish does it.
  const bool early = box && ntiles && !rem;
  const FinArgs fin = {c->ctl, nullptr, 0, early ? c->box_dev : nullptr, seq, nullptr};
  if (ntiles) {
    launch_decompress<T>(p, mode, grid, fin, geom, s, memo);
    if (memo) { c->memo_decodes++; SET_LAST(c, 1, "k_decompress_il<%s, %d, %d, true>", tname<T>(), mode, Phases<T>::D); }
    else if (takes_interleaved(p, geom)) SET_LAST(c, 1, "k_decompress_il<%s, %d, %d>", tname<T>(), mode, Phases<T>::D);
    else SET_LAST(c, 1, "k_decompress<%s, %d, %d, %d>", tname<T>(), mode, Phases<T>::D, geom);
  }
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[3], s));
  if (rem) launch_decompress_rem<T>(p, mode, scale, rem, s);
  if (box && !early) launch_finish(c->ctl, nullptr, 0, c->box_dev, seq, s);
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev[4], s));
  HIPCHK(c, hipGetLastError());
  Ctl* hc = reinterpret_cast<Ctl*>(c->h_pin + PIN_CTL);
  if (box) {
    int rc = wait_seq(c, &c->box->seq_done, seq, "decompress");
    if (rc) return rc;
    c->ctl_dirty = 0;
    hc->error = c->box->error;
    if (c->profiling) HIPCHK(c, hipEventSynchronize(c->ev[4]));
  } else {
    HIPCHK(c, hipMemcpyAsync(hc, c->ctl, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  // (a refused call leaves its flag in the device's control block -- the kernels set it when they meet the under-run, which
  // may be after the host has its answer --: the next call clears the block first.  Found by
  // test_under_run_is_refused_on_the_large_array_path: a good call behind a refused one was refused as well.)
  if (hc->error) c->ctl_dirty = 1;
  if (memo && hc->error == DEC_ERR_MEMO_STALE) {    // the streams are not what the compress call left: the same call, counting first
    c->memo.valid = false;
    c->memo_redos++;
    return decompress_impl<T>(c, d_bin, d_dc, d_ac, ac_count, qtable_host, n, eb, sf, mode, d_out, geom, nd);
  }
  if (hc->error == 2) return fail(c, DCTZHIP_E_ARG, "bin_index flags more exact coefficients than ac_count provides");
  if (hc->error) return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", hc->error);
  if (c->profiling) { int rc = read_timings(c, 2); if (rc) return rc; }
  return DCTZHIP_OK;
}

extern "C" int dctzhip_decompress(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac,
                                  uint32_t ac_count, const void* qtable_host, size_t n, int dtype, double eb, double sf,
                                  int mode, void* d_out) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  if (!d_bin || !d_dc || !d_out || (ac_count && !d_ac)) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_bin) || !aligned16(d_out)) return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  if (((uintptr_t)d_dc & 3u) || ((uintptr_t)d_ac & 3u)) return fail(c, DCTZHIP_E_ARG, "DC and AC_exact must be 4-byte aligned");
  if (mode == DCTZHIP_QT && !qtable_host) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
  {
    Span sp[4];
    size_t m = 0;
    decompress_spans(sp, &m, 0, d_bin, d_dc, d_ac, ac_count, n, dtype, d_out);
    rc = check_spans(c, sp, m, "dctzhip_decompress", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_scratch(c, n, dtype, DCTZHIP_EC, false);
  if (rc) return rc;
  rc = (dtype == DCTZHIP_F64)
           ? decompress_impl<double>(c, (const uint8_t*)d_bin, d_dc, d_ac, ac_count, qtable_host, n, eb, sf, mode, (double*)d_out)
           : decompress_impl<float>(c, (const uint8_t*)d_bin, d_dc, d_ac, ac_count, qtable_host, n, eb, sf, mode, (float*)d_out);
  if (rc == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

// ---- random access on decode (include/dctz_hip.h; dctz_kernels_ra.hip) ------------------------------------------
extern "C" size_t dctzhip_ac_index_len(size_t n) { return (n + DCTZHIP_INDEX_STRIDE - 1) / DCTZHIP_INDEX_STRIDE + 1; }

extern "C" int dctzhip_ac_index(dctzhip_ctx* c, const void* d_bin, size_t n, uint32_t* d_index, uint32_t* total) {
  if (!c) return DCTZHIP_E_ARG;
  if (n == 0 || n > (size_t)INT_MAX) return fail(c, DCTZHIP_E_ARG, "dctzhip_ac_index: n must be in [1, INT_MAX]");
  if (!d_bin || !d_index) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_bin) || ((uintptr_t)d_index & 3u)) return fail(c, DCTZHIP_E_ARG, "bin_index must be 16-byte aligned, the index 4-byte aligned");
  const size_t m = dctzhip_ac_index_len(n) - 1;
  {
    Span sp[2];
    size_t k = 0;
    add_span(sp, &k, d_bin, n, SPAN_READ, 0);
    add_span(sp, &k, d_index, (m + 1) * sizeof(uint32_t), SPAN_OUT, 0);
    int rc = check_spans(c, sp, k, "dctzhip_ac_index", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = regrow(c, &c->ix_part, &c->ix_part_cap, (m + IX_TPW - 1) / IX_TPW, sizeof(unsigned));
  if (rc) return rc;
  launch_ac_index((const uint8_t*)d_bin, (unsigned)n, d_index, c->ix_part, c->stream);
  HIPCHK(c, hipGetLastError());
  uint32_t* h = reinterpret_cast<uint32_t*>(c->h_pin + PIN_STATS);
  HIPCHK(c, hipMemcpyAsync(h, d_index + m, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (total) *total = *h;
  return DCTZHIP_OK;
}

namespace {
// the arguments that describe the streams, as an entry point gets them (host only)
struct StreamSet {
  const uint8_t* bin;
  const float* dc;
  const float* ac;
  uint32_t ac_count;
  const uint32_t* index;
  const void* qtable;             // on the host, 64 entries of the data type (QT mode)
  size_t n;                       // positions the streams cover: the elements of a flat array, 64 per block of a tiled one
  int dtype;
  double eb, sf;
  int mode;
};
}
// The streams are given and aligned and QT mode has its table (none of these messages names the entry point).  and_out: what
// the alignment message says beside bin_index -- "", or the call's output(s); has_out: d_out is the call's one output, to be
// given and 16-byte aligned like bin_index.
static int streams_given(dctzhip_ctx* c, const StreamSet& st, const char* and_out, bool has_out = false, const void* d_out = nullptr) {
  if (!st.bin || !st.dc || !st.index || (has_out && !d_out) || (st.ac_count && !st.ac)) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(st.bin) || !aligned16(d_out) || ((uintptr_t)st.dc & 3u) || ((uintptr_t)st.ac & 3u) || ((uintptr_t)st.index & 3u))
    return fail(c, DCTZHIP_E_ARG, "bin_index%s must be 16-byte aligned, DC, AC_exact and the index 4-byte aligned", and_out);
  if (st.mode == DCTZHIP_QT && !st.qtable) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
  return DCTZHIP_OK;
}
// What the stream tiles [t0, t1) read of bin_index, DC and the index: the tiles' positions [b0, b1), the DC of every block
// that has one of them, the index entries t0 .. t1.  (AC_exact is the caller's line, all of it: where a tile's part starts is
// only known on the device.)  The whole array is [0, ceil(n / TILE_ELEMS)): b0 = 0, b1 = n -- n bytes of bin_index,
// (n + 63) / 64 DC values, dctzhip_ac_index_len(n) index entries.  Of a tiled array n, so b1, is a multiple of 64 and the DC
// count is b1 / 64 - b0 / 64.
static void tile_read_spans(Span* sp, size_t* m, const StreamSet& st, size_t t0, size_t t1, int item) {
  const size_t b0 = t0 * TILE_ELEMS, b1 = std::min(st.n, t1 * (size_t)TILE_ELEMS);
  add_span(sp, m, st.bin + b0, b1 - b0, SPAN_READ, item);
  add_span(sp, m, st.dc + b0 / 64, ((b1 + 63) / 64 - b0 / 64) * sizeof(float), SPAN_READ, item);
  add_span(sp, m, st.index + t0, (t1 - t0 + 1) * sizeof(uint32_t), SPAN_READ, item);
}
static_assert(DCTZHIP_INDEX_STRIDE == TILE_ELEMS && TILE_ELEMS % 64 == 0, "index entries are per stream tile, tiles hold whole blocks");
// The buffers of a call with one output against each other: what the stream tiles [t0, t1) read, AC_exact, the output.
static int ra_check_spans(dctzhip_ctx* c, const char* what, const StreamSet& st, size_t t0, size_t t1, const void* d_out, size_t out_bytes) {
  Span sp[5];
  size_t m = 0;
  tile_read_spans(sp, &m, st, t0, t1, 0);
  add_span(sp, &m, st.ac, (size_t)st.ac_count * sizeof(float), SPAN_READ, 0);
  add_span(sp, &m, d_out, out_bytes, SPAN_OUT, 0);
  return check_spans(c, sp, m, what, nullptr);
}

// What the random-access calls share around their launch.  ra_begin: the control block is clean and the QT table staged;
// ra_fill: the fields every parameter block has; ra_finish: the error word read back -- the call returns once the index
// check is known, and has synchronised the stream.
template <typename T>
static int ra_begin(dctzhip_ctx* c, int mode, const void* qtable_host) {
  hipStream_t s = c->stream;
  if (c->ctl_dirty) HIPCHK(c, hipMemsetAsync(c->ctl, 0, sizeof(Ctl), s));
  c->ctl_dirty = 1;                                 // until this call's error word has been read back clean
  if (mode == DCTZHIP_QT) {
    // staged through pinned memory that the next call may rewrite: the call ends with a stream synchronisation
    T* hq = reinterpret_cast<T*>(c->h_pin + PIN_TAB + sizeof(double) * RTAB_SIZE);
    memcpy(hq, qtable_host, sizeof(T) * 64);
    HIPCHK(c, hipMemcpyAsync(c->qtab, hq, sizeof(T) * 64, hipMemcpyHostToDevice, s));
  }
  return DCTZHIP_OK;
}
template <typename T, typename P>
static void ra_fill_streams(dctzhip_ctx* c, P& p, const StreamSet& st) {
  p.bin = st.bin; p.dc = st.dc; p.ac = st.ac; p.idx = st.index;
  p.tab = tab_of<T>(c); p.qtab = reinterpret_cast<const T*>(c->qtab);
  p.ctl = c->ctl;
  p.ac_count = st.ac_count;
  p.sf = (T)st.sf;
  set_quant(p, inv_quant<T>(st.eb));
  p.eb = st.eb;
}
template <typename T, typename P>
static void ra_fill(dctzhip_ctx* c, P& p, const StreamSet& st, T* d_out) {
  ra_fill_streams<T>(c, p, st);
  p.out = d_out;
}
// cnt_total (or null): the control block's counter of the same read-back; a call that used it leaves the block to be cleared
static int ra_finish(dctzhip_ctx* c, unsigned* cnt_total = nullptr) {
  hipStream_t s = c->stream;
  HIPCHK(c, hipGetLastError());
  Ctl* hc = reinterpret_cast<Ctl*>(c->h_pin + PIN_CTL);
  HIPCHK(c, hipMemcpyAsync(hc, c->ctl, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (cnt_total) *cnt_total = hc->cnt_total;
  if (!hc->error && !cnt_total) c->ctl_dirty = 0;
  if (hc->error == 2) return fail(c, DCTZHIP_E_ARG, "the exception index disagrees with bin_index or exceeds ac_count");
  if (hc->error == 4) return fail(c, DCTZHIP_E_ARG, "the boxes hit more tiles than the bound of the work list");
  if (hc->error == 5) return fail(c, DCTZHIP_E_ARG, "the correction list contradicts itself or the array (fix_start, count or an offset)");
  if (hc->error) return fail(c, DCTZHIP_E_INTERNAL, "in-kernel error flag set (code %u)", hc->error);
  return DCTZHIP_OK;
}
// The grid of a launch with one single-wave workgroup per unit of work, persistent only beyond what is resident at once.
// What a unit is -- a candidate tile, a stream tile, a list item -- is said at the call.  slot: the context's (so its
// device's) cache of the kernel's resident workgroups per CU, 0 = not asked yet; occupancy() asks.
template <typename F>
static unsigned resident_grid(dctzhip_ctx* c, int& slot, size_t units, F occupancy) {
  if (slot == 0) slot = std::max(occupancy(), 1);
  const size_t resident = (size_t)c->num_cu * (size_t)slot;
  return (unsigned)(units < resident ? units : resident);
}

template <typename T>
static int decompress_range_impl(dctzhip_ctx* c, const StreamSet& st, size_t lo, size_t hi, T* d_out) {
  hipStream_t s = c->stream;
  const size_t n = st.n;
  const int mode = st.mode;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned t0 = (unsigned)(lo / TILE_ELEMS), t1 = (unsigned)((hi + TILE_ELEMS - 1) / TILE_ELEMS);
  const bool with_rem = rem && hi > (size_t)nfull * 64;
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  if (with_rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
  RangeParams<T> p;
  ra_fill<T>(c, p, st, d_out);
  p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.n = (unsigned)n; p.nfull = nfull; p.lo = (unsigned)lo; p.hi = (unsigned)hi; p.t0 = t0; p.t1 = t1;
  // a workgroup per tile of the range
  const int grid = (int)resident_grid(c, c->ra_occ[sizeof(T) == 8][mode == DCTZHIP_QT], t1 - t0, [&] { return range_occupancy<T>(mode); });
  // (no stage timings: dctzhip_last_timings keeps reporting the last compress / decompress call)
  launch_decompress_range<T>(p, mode, grid, with_rem, s);
  SET_LAST(c, 1, "k_decompress_range<%s, %d>", tname<T>(), mode);
  return ra_finish(c);
}

extern "C" int dctzhip_decompress_range(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                        const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf,
                                        int mode, size_t lo, size_t hi, void* d_out) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  if (lo >= hi || hi > n) return fail(c, DCTZHIP_E_ARG, "dctzhip_decompress_range: the range [%zu, %zu) is not inside [0, %zu)", lo, hi, n);
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  if ((rc = streams_given(c, st, " and the output", true, d_out))) return rc;
  // what the call reads: the range's tiles and AC_exact
  rc = ra_check_spans(c, "dctzhip_decompress_range", st, lo / TILE_ELEMS, (hi + TILE_ELEMS - 1) / TILE_ELEMS, d_out, (hi - lo) * elem_size(dtype));
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64) ? decompress_range_impl<double>(c, st, lo, hi, (double*)d_out)
                                : decompress_range_impl<float>(c, st, lo, hi, (float*)d_out);
}

// ---- a box of an N-D array (include/dctz_hip.h; dctz_kernels_box.hip) -------------------------------------------
// The box in its canonical form: dimensions of size 1 drop out, a dimension the box covers completely merges into the
// one in front of it (coordinates (a, b) -> a D + b, the box's [lo, hi) x [0, D) -> [lo D, hi D): the runs become as long
// as the box allows), the rest is padded in front with dimensions of size 1.  The arguments have been checked.
static BoxGeo canonical_box(int ndim, const size_t* dims, const size_t* lo, const size_t* hi) {
  size_t d[DCTZHIP_BOX_MAXDIM], l[DCTZHIP_BOX_MAXDIM], h[DCTZHIP_BOX_MAXDIM];
  int k = 0;
  for (int i = 0; i < ndim; i++) {
    if (dims[i] == 1) continue;
    if (k > 0 && lo[i] == 0 && hi[i] == dims[i]) { d[k - 1] *= dims[i]; l[k - 1] *= dims[i]; h[k - 1] *= dims[i]; continue; }
    d[k] = dims[i]; l[k] = lo[i]; h[k] = hi[i]; k++;
  }
  BoxGeo g;
  for (int i = 0; i < BOX_ND; i++) {
    const int j = i - (BOX_ND - k);
    g.dim[i] = j >= 0 ? (unsigned)d[j] : 1u;
    g.lo[i] = j >= 0 ? (unsigned)l[j] : 0u;
    g.ext[i] = j >= 0 ? (unsigned)(h[j] - l[j]) : 1u;
  }
  unsigned q = 64u;                                  // a wave row of output positions in the mixed radix of ext
  for (int i = BOX_ND - 1; i > 0; i--) { g.step[i] = q % g.ext[i]; q /= g.ext[i]; }
  g.step[0] = q;
  unsigned stride[BOX_ND];
  stride[BOX_ND - 1] = 1u;
  for (int i = BOX_ND - 1; i > 0; i--) stride[i - 1] = stride[i] * g.dim[i];
  g.fstep = 0u;
  for (int i = 0; i < BOX_ND; i++) g.fstep += g.step[i] * stride[i];
  g.wrap[0] = 0u;
  for (int i = 1; i < BOX_ND; i++) g.wrap[i] = stride[i - 1] - g.ext[i] * stride[i];
  return g;
}

// The extents of one box against the array (dims are checked with it): its element count, first and last flat element.
static int box_extents(dctzhip_ctx* c, const char* what, size_t n, int ndim, const size_t* dims, const size_t* lo, const size_t* hi,
                       size_t* cnt, size_t* first, size_t* last) {
  size_t prod = 1;
  *cnt = 1; *first = 0; *last = 0;
  for (int i = 0; i < ndim; i++) {
    // (n <= INT_MAX: a product that stays <= n cannot overflow)
    if (dims[i] == 0 || dims[i] > n / prod) return fail(c, DCTZHIP_E_ARG, "%s: the product of dims is not n = %zu", what, n);
    prod *= dims[i];
    if (lo[i] >= hi[i] || hi[i] > dims[i])
      return fail(c, DCTZHIP_E_ARG, "%s: [%zu, %zu) is not inside dimension %d of %zu", what, lo[i], hi[i], i, dims[i]);
    *cnt *= hi[i] - lo[i];
    *first = *first * dims[i] + lo[i];
    *last = *last * dims[i] + (hi[i] - 1);
  }
  if (prod != n) return fail(c, DCTZHIP_E_ARG, "%s: the product of dims is not n = %zu", what, n);
  return DCTZHIP_OK;
}
// The box arguments of a call with one box of a flat array: the rank, the arrays, then the extents.
static int box_front(dctzhip_ctx* c, const char* what, size_t n, int ndim, const size_t* dims, const size_t* lo, const size_t* hi,
                     size_t* cnt, size_t* first, size_t* last) {
  if (ndim < 1 || ndim > DCTZHIP_BOX_MAXDIM) return fail(c, DCTZHIP_E_ARG, "%s: ndim must be in [1, %d]", what, DCTZHIP_BOX_MAXDIM);
  if (!dims || !lo || !hi) return fail(c, DCTZHIP_E_ARG, "%s: null dims, lo or hi", what);
  return box_extents(c, what, n, ndim, dims, lo, hi, cnt, first, last);
}

// [first, last]: the box's first and last flat element -- the candidate tiles are those of the range [first, last + 1)
template <typename T>
static int decompress_box_impl(dctzhip_ctx* c, const StreamSet& st, const BoxGeo& box, size_t first, size_t last, T* d_out) {
  hipStream_t s = c->stream;
  const size_t n = st.n;
  const int mode = st.mode;
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  const unsigned t0 = (unsigned)(first / TILE_ELEMS), t1 = (unsigned)(last / TILE_ELEMS + 1);
  const bool with_rem = rem && box.rank((unsigned)n) != box.rank(nfull * 64u);    // an element of the short block lies in the box
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  if (with_rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
  BoxParams<T> p;
  ra_fill<T>(c, p, st, d_out);
  p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.n = (unsigned)n; p.nfull = nfull; p.t0 = t0; p.t1 = t1;
  p.box = box;
  // a workgroup per candidate tile
  const unsigned tiles = t1 - t0;
  const int grid = (int)resident_grid(c, c->box_occ[sizeof(T) == 8][mode == DCTZHIP_QT], tiles, [&] { return box_occupancy<T>(mode); });
  c->box_grid = (unsigned)grid; c->box_tiles = tiles;
  launch_decompress_box<T>(p, mode, grid, with_rem, s);
  SET_LAST(c, 1, "k_decompress_box<%s, %d>", tname<T>(), mode);
  return ra_finish(c);
}

extern "C" int dctzhip_decompress_box(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                      const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf,
                                      int mode, int ndim, const size_t* dims, const size_t* lo, const size_t* hi, void* d_out) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  size_t cnt = 1, first = 0, last = 0;
  rc = box_front(c, "dctzhip_decompress_box", n, ndim, dims, lo, hi, &cnt, &first, &last);
  if (rc) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  if ((rc = streams_given(c, st, " and the output", true, d_out))) return rc;
  // what the call may read: what dctzhip_decompress_range reads for [first box element, last box element + 1)
  rc = ra_check_spans(c, "dctzhip_decompress_box", st, first / TILE_ELEMS, last / TILE_ELEMS + 1, d_out, cnt * elem_size(dtype));
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const BoxGeo box = canonical_box(ndim, dims, lo, hi);
  return (dtype == DCTZHIP_F64) ? decompress_box_impl<double>(c, st, box, first, last, (double*)d_out)
                                : decompress_box_impl<float>(c, st, box, first, last, (float*)d_out);
}

// ---- multi-dimensional blocks (include/dctz_hip.h) -------------------------------------------------
static bool nd_shape(int ndims, const size_t* dims, NdShape* sh) {
  if ((ndims != 2 && ndims != 3) || !dims) return false;
  const size_t edge = ndims == 2 ? 8 : 4;
  sh->nd = ndims;
  sh->nblk = 1;
  for (int i = 0; i < 3; i++) { sh->d[i] = 1; sh->nb[i] = 1; }
  for (int i = 0; i < ndims; i++) {
    if (dims[i] == 0 || dims[i] > (size_t)INT_MAX) return false;
    sh->d[i] = dims[i];
    sh->nb[i] = (dims[i] + edge - 1) / edge;
    if (sh->nblk > (size_t)INT_MAX / 64 / sh->nb[i]) return false;        // nblk * 64 must stay an int (dctz.h:126)
    sh->nblk *= sh->nb[i];
  }
  return true;
}

extern "C" size_t dctzhip_nd_blocks(int ndims, const size_t* dims) {
  NdShape sh;
  return nd_shape(ndims, dims, &sh) ? sh.nblk : 0;
}
// How every entry point for a tiled array opens: the context, the shape, then dtype, mode and the 64 sh->nblk stream positions.
static int nd_front(dctzhip_ctx* c, int ndims, const size_t* dims, int dtype, int mode, NdShape* sh) {
  if (!c) return DCTZHIP_E_ARG;
  if (!nd_shape(ndims, dims, sh)) return fail(c, DCTZHIP_E_ARG, "multi-dimensional blocks: 2 or 3 non-zero extents whose tile count fits an int");
  return check_common(c, sh->nblk * 64, dtype, mode);
}
// The box [lo, hi) of a tiled array: inside the array, cnt its elements, [t0, t1) the stream tiles from the one of its first
// intersecting block to the one of its last (blocks in the row-major order of the block grid).  cell != 0: sh.d are coarse
// extents and a block owns `cell` of their cells per axis (sh.nb is still the block grid).
static int nd_box_front(dctzhip_ctx* c, const char* what, const NdShape& sh, const size_t* lo, const size_t* hi, size_t* cnt, unsigned* t0,
                        unsigned* t1, size_t cell = 0) {
  if (!lo || !hi) return fail(c, DCTZHIP_E_ARG, "%s: null lo or hi", what);
  const size_t edge = cell ? cell : sh.nd == 2 ? 8 : 4;
  size_t first = 0, last = 0;
  *cnt = 1;
  for (int i = 0; i < sh.nd; i++) {
    if (lo[i] >= hi[i] || hi[i] > sh.d[i])
      return fail(c, DCTZHIP_E_ARG, "%s: [%zu, %zu) is not inside dimension %d of %zu", what, lo[i], hi[i], i, sh.d[i]);
    *cnt *= hi[i] - lo[i];
    first = first * sh.nb[i] + lo[i] / edge;
    last = last * sh.nb[i] + (hi[i] - 1) / edge;
  }
  *t0 = (unsigned)(first / TILE_BLKS); *t1 = (unsigned)(last / TILE_BLKS + 1);
  return DCTZHIP_OK;
}
// value(0 .. nd - 1) in the last nd of three axes, `front` in the axes before them: how the kernels take a tiled array or a box of one
template <typename F>
static void last_axes(int nd, unsigned (&a)[3], unsigned front, F value) {
  for (int i = 0; i < 3; i++) a[i] = i < 3 - nd ? front : (unsigned)value(i - (3 - nd));
}

// The kernels can read / write the array in place (NdDirect) when no tile is padded and one 32-bit buffer descriptor
// covers it; DCTZHIP_ND_DIRECT=0 forces the gather / scatter passes (A/B, tests).
static bool nd_direct(dctzhip_ctx* c, const NdShape& sh, size_t es, NdDirect* d) {
  memset(d, 0, sizeof(*d));
  if (!c->nd_direct) return false;
  const size_t edge = sh.nd == 2 ? 8 : 4;
  size_t n = 1;
  for (int i = 0; i < sh.nd; i++) { if (sh.d[i] % edge) return false; n *= sh.d[i]; }
  if (n * es > (size_t)0xFFFFF000u) return false;
  d->on = 1; d->nd = (unsigned)sh.nd;
  d->dx = (unsigned)sh.d[sh.nd - 1]; d->dy = sh.nd == 3 ? (unsigned)sh.d[1] : 1u;
  d->nbx = (unsigned)sh.nb[sh.nd - 1]; d->nby = sh.nd == 3 ? (unsigned)sh.nb[1] : 1u;
  d->mx = (unsigned)(((unsigned long long)1 << 32) / d->nbx > 0xFFFFFFFFull ? 0xFFFFFFFFull : ((unsigned long long)1 << 32) / d->nbx);
  d->my = (unsigned)(((unsigned long long)1 << 32) / d->nby > 0xFFFFFFFFull ? 0xFFFFFFFFull : ((unsigned long long)1 << 32) / d->nby);
  d->nblk = (unsigned)sh.nblk;
  d->bytes = (unsigned)(n * es);
  return true;
}

static int ensure_nd(dctzhip_ctx* c, size_t bytes) {
  char* b = (char*)c->nd_buf;
  int rc = regrow(c, &b, &c->nd_cap, bytes, 1);
  c->nd_buf = b;
  return rc;
}

template <typename T>
static int compress_nd_impl(dctzhip_ctx* c, const T* d_in, const NdShape& sh, double eb, int mode, uint8_t* d_bin,
                            float* d_dc, float* d_ac, T* d_scaled, dctzhip_cinfo* info) {
  const size_t n_lin = sh.nblk * 64, n_orig = sh.d[0] * sh.d[1] * sh.d[2];
  NdDirect direct;
  if (nd_direct(c, sh, sizeof(T), &direct))         // no padding, below 4 GiB: the flat pipeline with other addresses
    return compress_impl<T>(c, d_in, n_orig, eb, mode, d_bin, d_dc, d_ac, d_scaled, (T*)nullptr, info, sh.nd == 2 ? GEOM_2D : GEOM_3D, 0,
                            n_orig, &direct);
  int rc = ensure_nd(c, n_lin * sizeof(T));
  if (rc) return rc;
  T* lin = reinterpret_cast<T*>(c->nd_buf);
  // tiles -> block after block, with calc_data_stat's reductions over the original elements on the way
  const size_t nq = n_lin / Traits<T>::EPV;
  int grid = (int)((nq + SWG * 4 - 1) / (SWG * 4));
  if (grid < 1) grid = 1;
  if (grid > c->stats_grid) grid = c->stats_grid;
  launch_gather_nd<T>(d_in, lin, sh, c->part, grid, c->stream);
  HIPCHK(c, hipGetLastError());
  dctzhip_cinfo local;
  rc = compress_impl<T>(c, lin, n_lin, eb, mode, d_bin, d_dc, d_ac, (T*)nullptr, (T*)nullptr, &local, sh.nd == 2 ? GEOM_2D : GEOM_3D,
                        grid, n_orig);
  if (rc) return rc;
  if (d_scaled) {                                   // dctz-comp-lib.c:193-216 on the caller's array
    const T sf_t = (T)local.sf;
    if (sf_t != (T)1.0) launch_scale<T>(d_in, d_scaled, n_orig, sf_t, c->num_cu * 8, c->stream);
    else if ((const void*)d_scaled != (const void*)d_in) HIPCHK(c, hipMemcpyAsync(d_scaled, d_in, n_orig * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipGetLastError());
  }
  if (info) *info = local;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_compress_nd(dctzhip_ctx* c, const void* d_in, int ndims, const size_t* dims, int dtype, double eb,
                                   int mode, void* d_bin, float* d_dc, float* d_ac, void* d_scaled, dctzhip_cinfo* info) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  if (!d_in || !d_bin || !d_dc || !d_ac) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_in) || !aligned16(d_bin) || !aligned16(d_dc) || !aligned16(d_ac) || (d_scaled && !aligned16(d_scaled)))
    return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  if (eb < 1E-6) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_scratch(c, sh.nblk * 64, dtype, mode);
  if (rc) return rc;
  rc = (dtype == DCTZHIP_F64)
           ? compress_nd_impl<double>(c, (const double*)d_in, sh, eb, mode, (uint8_t*)d_bin, d_dc, d_ac, (double*)d_scaled, info)
           : compress_nd_impl<float>(c, (const float*)d_in, sh, eb, mode, (uint8_t*)d_bin, d_dc, d_ac, (float*)d_scaled, info);
  if (rc == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

template <typename T>
static int decompress_nd_impl(dctzhip_ctx* c, const uint8_t* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                              const void* qtable_host, const NdShape& sh, double eb, double sf, int mode, T* d_out) {
  const size_t n_lin = sh.nblk * 64;
  const int geom = sh.nd == 2 ? GEOM_2D : GEOM_3D;
  NdDirect direct;
  if (nd_direct(c, sh, sizeof(T), &direct))         // no padding, below 4 GiB: the flat pipeline with other addresses
    return decompress_impl<T>(c, d_bin, d_dc, d_ac, ac_count, qtable_host, n_lin, eb, sf, mode, d_out, geom, &direct);
  int rc = ensure_nd(c, n_lin * sizeof(T));
  if (rc) return rc;
  T* lin = reinterpret_cast<T*>(c->nd_buf);
  rc = decompress_impl<T>(c, d_bin, d_dc, d_ac, ac_count, qtable_host, n_lin, eb, sf, mode, lin, geom);
  if (rc) return rc;
  // block after block -> tiles
  launch_scatter_nd<T>(lin, d_out, sh, c->num_cu * 8, c->stream);
  HIPCHK(c, hipGetLastError());
  return DCTZHIP_OK;
}

extern "C" int dctzhip_decompress_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                     const void* qtable_host, int ndims, const size_t* dims, int dtype, double eb, double sf,
                                     int mode, void* d_out) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  if (!d_bin || !d_dc || !d_out || (ac_count && !d_ac)) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_bin) || !aligned16(d_out)) return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  if (((uintptr_t)d_dc & 3u) || ((uintptr_t)d_ac & 3u)) return fail(c, DCTZHIP_E_ARG, "DC and AC_exact must be 4-byte aligned");
  if (mode == DCTZHIP_QT && !qtable_host) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
  HIPCHK(c, hipSetDevice(c->device));
  rc = ensure_scratch(c, sh.nblk * 64, dtype, DCTZHIP_EC, false);
  if (rc) return rc;
  rc = (dtype == DCTZHIP_F64)
           ? decompress_nd_impl<double>(c, (const uint8_t*)d_bin, d_dc, d_ac, ac_count, qtable_host, sh, eb, sf, mode, (double*)d_out)
           : decompress_nd_impl<float>(c, (const uint8_t*)d_bin, d_dc, d_ac, ac_count, qtable_host, sh, eb, sf, mode, (float*)d_out);
  if (rc == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return rc;
}

// ---- a box of an array compressed in tiles (include/dctz_hip.h; dctz_kernels_ndbox.hip) -------------------------
// The checked box [lo, hi) as the kernels take it: the array in the last sh.nd of three axes (nb: blocks per axis; blo, ext:
// the box in elements), and the intersecting blocks as a box of the block grid (dim = nb; rank() is the hit test).  cell: as
// for nd_box_front.
static void nd_box_geometry(const NdShape& sh, const size_t* lo, const size_t* hi, unsigned (&nb)[3], unsigned (&blo)[3], unsigned (&ext)[3],
                            BoxGeo* blocks, unsigned cell = 0) {
  const unsigned edge = cell ? cell : sh.nd == 2 ? 8u : 4u;
  memset(blocks, 0, sizeof(*blocks));
  for (int i = 0; i < BOX_ND; i++) { blocks->dim[i] = 1u; blocks->lo[i] = 0u; blocks->ext[i] = 1u; }
  for (int i = 0; i < 3; i++) { nb[i] = 1u; blo[i] = 0u; ext[i] = 1u; }
  for (int i = 0; i < sh.nd; i++) {
    const int a = 3 - sh.nd + i;
    nb[a] = (unsigned)sh.nb[i]; blo[a] = (unsigned)lo[i]; ext[a] = (unsigned)(hi[i] - lo[i]);
    const unsigned bl = (unsigned)lo[i] / edge, bh = (unsigned)(hi[i] - 1) / edge;
    blocks->dim[a + 1] = (unsigned)sh.nb[i]; blocks->lo[a + 1] = bl; blocks->ext[a + 1] = bh - bl + 1u;
  }
}

template <typename T>
static int decompress_box_nd_impl(dctzhip_ctx* c, const StreamSet& st, const NdShape& sh, const size_t* lo, const size_t* hi, unsigned t0,
                                  unsigned t1, T* d_out) {
  hipStream_t s = c->stream;
  const int mode = st.mode;
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  NdBoxParams<T> p;
  ra_fill<T>(c, p, st, d_out);
  p.n = (unsigned)(sh.nblk * 64); p.nfull = (unsigned)sh.nblk; p.t0 = t0; p.t1 = t1;
  nd_box_geometry(sh, lo, hi, p.nb, p.lo, p.ext, &p.blocks);
  // a workgroup per candidate tile
  const int geom = sh.nd == 2 ? GEOM_2D : GEOM_3D;
  const unsigned tiles = t1 - t0;
  int grid = (int)resident_grid(c, c->ndbox_occ[sizeof(T) == 8][mode == DCTZHIP_QT][sh.nd == 3], tiles, [&] { return ndbox_occupancy<T>(mode, geom); });
  // A heuristic, measured on two boxes of one volume only: the stride of the loop over tiles is kept ODD.  The hit tiles
  // of a box repeat with the tiles per block row and per block plane, even numbers for most shapes; with the even stride
  // 1024 the x-plane of a 512^3 volume (every other tile is hit) left half of the workgroups without a single hit tile:
  // 254 -> 142 us.  It does not balance the 64^3 brick (a workgroup still meets four hit tiles) and costs the full box
  // 3.5 % (369 -> 382 us).  An assignment that follows the hit tiles instead of the candidates is the real fix (EXPERIMENTS
  // section 22).
  if (tiles > (unsigned)grid && grid > 1 && !(grid & 1)) grid--;       // (more tiles than the grid: the workgroups are persistent)
  c->box_grid = (unsigned)grid; c->box_tiles = tiles;
  launch_decompress_ndbox<T>(p, mode, geom, grid, s);
  SET_LAST(c, 1, "k_decompress_ndbox<%s, %d, %d>", tname<T>(), mode, geom);
  return ra_finish(c);
}

extern "C" int dctzhip_decompress_box_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                         const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims, int dtype,
                                         double eb, double sf, int mode, const size_t* lo, const size_t* hi, void* d_out) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  size_t cnt = 1;
  unsigned t0 = 0, t1 = 0;
  if ((rc = nd_box_front(c, "dctzhip_decompress_box_nd", sh, lo, hi, &cnt, &t0, &t1))) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, sh.nblk * 64, dtype, eb, sf, mode};
  if ((rc = streams_given(c, st, " and the output", true, d_out))) return rc;
  // what the call may read: the candidate tiles and AC_exact
  if ((rc = ra_check_spans(c, "dctzhip_decompress_box_nd", st, t0, t1, d_out, cnt * elem_size(dtype)))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64) ? decompress_box_nd_impl<double>(c, st, sh, lo, hi, t0, t1, (double*)d_out)
                                : decompress_box_nd_impl<float>(c, st, sh, lo, hi, t0, t1, (float*)d_out);
}

// ---- a list of boxes in one call (include/dctz_hip.h; dctz_kernels_mbox.hip, tiled: dctz_kernels_mboxnd.hip) -----
static constexpr size_t MBOX_LIST_MAX = (size_t)1 << 24;                // items: the bound B of a call may not exceed it
// the table of a call: the records, then per box an unsigned (flat arrays: the boxes of the short block) or the box in elements (tiled arrays)
static constexpr size_t MBOX_TABLE_BYTES = (size_t)DCTZHIP_BOXES_MAX * (sizeof(BoxRec) + std::max(sizeof(unsigned), sizeof(NdBoxElems)));
static int mbox_table(dctzhip_ctx* c) {
  if (!c->mb_pin) {
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->mb_pin), MBOX_TABLE_BYTES, hipHostMallocDefault));
    HIPCHK(c, hipMalloc(&c->mb_dev, MBOX_TABLE_BYTES));
  }
  return DCTZHIP_OK;
}

// sh null: st.n elements in flat blocks; else the tiles of sh (st.n = 64 sh->nblk, no short block).  recs[0, k) are complete
// but for the device side of the table; side[0, side_bytes) is the table's second half -- flat: the boxes that reach into
// the short block, an unsigned each; tiled: the k boxes in elements, an NdBoxElems each; B bounds the hits.
// cz (or null): the boxes are of the coarse decode -- sh is the coarse shape, the boxes are in its cells, cz->k per block and
// axis; with cz->k == 1 there is no list (B = 0): one gather from the DC stream, cz->max_cells the cells of the largest box.
namespace {
struct CoarseZoom { int factor, k; unsigned max_cells; };
}
template <typename T>
static int decompress_boxes_impl(dctzhip_ctx* c, const StreamSet& st, const NdShape* sh, int k, const BoxRec* recs, const void* side,
                                 size_t side_bytes, unsigned total, size_t B, const CoarseZoom* cz = nullptr) {
  hipStream_t s = c->stream;
  const int mode = st.mode;
  const int nrem = sh ? 0 : (int)(side_bytes / sizeof(unsigned));
  int rc;
  if ((rc = mbox_table(c))) return rc;
  if (B && (rc = regrow(c, &c->mb_items, &c->mb_items_cap, B, sizeof(BoxItem)))) return rc;
  c->ctl_dirty = 1;                                  // the list's counter is the control block's: cleared in stream order, always
  if ((rc = ra_begin<T>(c, mode, st.qtable))) return rc;
  if (nrem) { if ((rc = upload_rtab<T>(c, (int)(st.n % 64)))) return rc; }      // (it can fail: in front of the table's copy)
  // the table in one transfer, on the call's stream, behind everything of the prologue that can fail: from here on the call
  // reaches its synchronisation (ra_finish), or the stream is synchronised before the error is returned, so the pinned
  // copy is never rewritten under a copy in flight
  const size_t rec_bytes = (size_t)k * sizeof(BoxRec);
  memcpy(c->mb_pin, recs, rec_bytes);
  memcpy(c->mb_pin + rec_bytes, side, side_bytes);
  {
    const hipError_t e = hipMemcpyAsync(c->mb_dev, c->mb_pin, rec_bytes + side_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(s);
      return fail(c, DCTZHIP_E_HIP, "copy of the box table failed: %s", hipGetErrorString(e));
    }
  }
  BoxListParams lp;
  lp.recs = reinterpret_cast<const BoxRec*>(c->mb_dev);
  lp.nbox = (unsigned)k; lp.total = total;
  lp.unit = (unsigned)(sh ? TILE_BLKS : TILE_ELEMS); lp.end = (unsigned)(sh ? sh->nblk : st.n);
  lp.items = c->mb_items; lp.cap = (unsigned)B; lp.ctl = c->ctl;
  // what the two parameter blocks share
  auto fill = [&](auto& p) {
    ra_fill_streams<T>(c, p, st);
    p.recs = lp.recs; p.items = c->mb_items;
    p.cap = (unsigned)B; p.n = (unsigned)st.n; p.nfull = (unsigned)(st.n / 64);
  };
  c->mbox_bound = (unsigned)B; c->mbox_items = 0;
  // workgroups that take items off the list: at most one per item the list can hold
  if (!sh) {
    MBoxParams<T> p;
    fill(p);
    p.rtab = reinterpret_cast<const T*>(c->rtab);
    p.rem_boxes = reinterpret_cast<const unsigned*>(c->mb_dev + rec_bytes);
    const int grid = (int)resident_grid(c, c->mbox_occ[sizeof(T) == 8][mode == DCTZHIP_QT], B, [&] { return mbox_occupancy<T>(mode); });
    c->mbox_grid = (unsigned)grid;
    launch_boxlist_build(lp, s);
    launch_decompress_mbox<T>(p, mode, grid, nrem, s);
    SET_LAST(c, 1, "k_decompress_mbox<%s, %d>", tname<T>(), mode);
  } else if (cz) {
    const int geom = sh->nd == 2 ? GEOM_2D : GEOM_3D;
    MCBoxNdParams<T> p;
    ra_fill<T>(c, p.c, st, (T*)nullptr);
    p.c.rtab = nullptr;
    p.c.n = (unsigned)st.n; p.c.nfull = (unsigned)sh->nblk; p.c.ntiles = (p.c.nfull + (unsigned)TILE_BLKS - 1u) / (unsigned)TILE_BLKS;
    p.c.factor = (unsigned)cz->factor;
    last_axes(sh->nd, p.c.nb, 1u, [&](int i) { return sh->nb[i]; });
    last_axes(sh->nd, p.c.od, 1u, [&](int i) { return sh->d[i]; });
    p.recs = lp.recs; p.items = c->mb_items; p.cap = (unsigned)B;
    p.elems = reinterpret_cast<const NdBoxElems*>(c->mb_dev + rec_bytes);
    if (cz->k == 1) {
      // the block grid is the output grid: every box from the DC stream alone, in one launch
      c->mbox_grid = launch_ndcoarse_mbox_dc<T>(st.dc, p.recs, p.elems, (unsigned)k, cz->max_cells, p.c.nb, (T)st.sf, s);
      SET_LAST(c, 1, "k_ndcoarse_mbox_dc<%s>", tname<T>());
    } else {
      // (DCTZHIP_WG_PER_CU sets the resident workgroups instead, as for the single call)
      int forced = c->wg_per_cu;
      int& occ = forced ? forced : c->mcboxnd_occ[sizeof(T) == 8][mode == DCTZHIP_QT][sh->nd == 3][cz->k == 4];
      const int grid = (int)resident_grid(c, occ, B, [&] { return mcboxnd_occupancy<T>(mode, geom, cz->k); });
      c->mbox_grid = (unsigned)grid;
      launch_boxlist_build(lp, s);
      launch_ndcoarse_mbox<T>(p, mode, geom, cz->k, grid, s);
      SET_LAST(c, 1, "k_ndcoarse_mbox<%s, %d, %d, %d>", tname<T>(), mode, geom, cz->k);
    }
  } else {
    const int geom = sh->nd == 2 ? GEOM_2D : GEOM_3D;
    MBoxNdParams<T> p;
    fill(p);
    p.elems = reinterpret_cast<const NdBoxElems*>(c->mb_dev + rec_bytes);
    last_axes(sh->nd, p.nb, 1u, [&](int i) { return sh->nb[i]; });
    const int grid = (int)resident_grid(c, c->mboxnd_occ[sizeof(T) == 8][mode == DCTZHIP_QT][sh->nd == 3], B, [&] { return mboxnd_occupancy<T>(mode, geom); });
    c->mbox_grid = (unsigned)grid;
    launch_boxlist_build(lp, s);
    launch_decompress_mbox_nd<T>(p, mode, geom, grid, s);
    SET_LAST(c, 1, "k_decompress_mbox_nd<%s, %d, %d>", tname<T>(), mode, geom);
  }
  rc = ra_finish(c, &c->mbox_items);
  if (rc == DCTZHIP_E_HIP) (void)hipStreamSynchronize(s);   // (a failed launch or read-back: the table's copy may still be in flight)
  return rc;
}

// What the entry points share from the k check on.  sh null: the flat array of st.n elements seen with the shape dims[0, ndim),
// which is checked here; else the tiles of sh.  factor != 0: the boxes of the coarse decode at that (checked) factor -- sh is
// the coarse shape over the array's own block grid, a block owns cell = edge / factor of its cells per axis; with cell == 1
// the DC stream alone is read, per box from its first to its last block, and the other streams may be missing.
static int decompress_boxes_call(dctzhip_ctx* c, const char* what, const StreamSet& st, const NdShape* sh, int ndim, const size_t* dims, int k,
                                 const dctzhip_box_item* boxes, int factor = 0, int cell = 0) {
  int rc;
  if (k < 1 || k > DCTZHIP_BOXES_MAX) return fail(c, DCTZHIP_E_ARG, "%s: k must be in [1, %d]", what, DCTZHIP_BOXES_MAX);
  if (!boxes) return fail(c, DCTZHIP_E_ARG, "%s: null boxes", what);
  if (!sh) {
    if (ndim < 1 || ndim > DCTZHIP_BOX_MAXDIM) return fail(c, DCTZHIP_E_ARG, "%s: ndim must be in [1, %d]", what, DCTZHIP_BOX_MAXDIM);
    if (!dims) return fail(c, DCTZHIP_E_ARG, "%s: null dims", what);
  }
  const bool dc_only = cell == 1;
  if (dc_only) {
    if (!st.dc) return fail(c, DCTZHIP_E_ARG, "null device buffer");
    if ((uintptr_t)st.dc & 3u) return fail(c, DCTZHIP_E_ARG, "DC must be 4-byte aligned");
    if (st.mode == DCTZHIP_QT && !st.qtable) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
  } else if ((rc = streams_given(c, st, " and the outputs"))) return rc;    // (the outputs themselves: box by box, below)
  const unsigned nfull = (unsigned)(st.n / 64);
  const bool rem = st.n % 64 != 0;
  const size_t unit = sh ? TILE_BLKS : TILE_ELEMS;  // what a candidate spans: the blocks, or of a flat array the elements, of a stream tile
  std::vector<BoxRec> recs((size_t)k);
  // the second half of the table: the boxes that reach into the short block (flat), or every box in elements (tiled)
  std::vector<unsigned> rem_boxes;
  std::vector<NdBoxElems> elems(sh ? (size_t)k : 0);
  // every buffer of the call against every other: the outputs may overlap nothing, neither each other nor what any box reads
  std::vector<Span> sp((size_t)k * 4 + 1);
  size_t m = 0, B = 0, total = 0, max_cells = 0;
  if (!dc_only) add_span(sp.data(), &m, st.ac, (size_t)st.ac_count * sizeof(float), SPAN_READ, -1);
  for (int i = 0; i < k; i++) {
    char box[56];
    snprintf(box, sizeof(box), "%s: box %d", what, i);
    size_t cnt = 1;
    BoxRec& r = recs[(size_t)i];
    if (!sh) {
      size_t first, last;
      if ((rc = box_extents(c, box, st.n, ndim, dims, boxes[i].lo, boxes[i].hi, &cnt, &first, &last))) return rc;
      r.t0 = (unsigned)(first / TILE_ELEMS); r.t1 = (unsigned)(last / TILE_ELEMS + 1);
      r.g = canonical_box(ndim, dims, boxes[i].lo, boxes[i].hi);
      if (rem && r.g.rank((unsigned)st.n) != r.g.rank(nfull * 64u)) rem_boxes.push_back((unsigned)i);
    } else {
      if ((rc = nd_box_front(c, box, *sh, boxes[i].lo, boxes[i].hi, &cnt, &r.t0, &r.t1, (size_t)cell))) return rc;
      unsigned nb[3];
      nd_box_geometry(*sh, boxes[i].lo, boxes[i].hi, nb, elems[(size_t)i].lo, elems[(size_t)i].ext, &r.g, (unsigned)cell);
    }
    if (!boxes[i].d_out) return fail(c, DCTZHIP_E_ARG, "%s: null output", box);
    if (!aligned16(boxes[i].d_out)) return fail(c, DCTZHIP_E_ARG, "%s: the output must be 16-byte aligned", box);
    if (dc_only) {
      // no candidates, no list: the DC words from the first to the last block of the box
      size_t first = 0, last = 0;
      for (int d = 0; d < sh->nd; d++) { first = first * sh->nb[d] + boxes[i].lo[d]; last = last * sh->nb[d] + (boxes[i].hi[d] - 1); }
      add_span(sp.data(), &m, st.dc + first, (last - first + 1) * sizeof(float), SPAN_READ, i);
      r.t0 = r.t1 = 0;
      max_cells = std::max(max_cells, cnt);
    } else {
      tile_read_spans(sp.data(), &m, st, r.t0, r.t1, i);
    }
    add_span(sp.data(), &m, boxes[i].d_out, cnt * elem_size(st.dtype), SPAN_OUT, i);
    r.cand0 = (unsigned)total;                      // (k <= 2^12 boxes of <= 2^19 candidates each)
    r.out = boxes[i].d_out;
    const size_t cand = r.t1 - r.t0;
    total += cand;
    // a run of L consecutive elements (blocks) touches at most ceil((L - 1) / unit) + 1 stream tiles
    size_t runs = 1;
    for (int d = 0; d < BOX_ND - 1; d++) runs *= r.g.ext[d];
    const size_t runlen = r.g.ext[BOX_ND - 1];
    B += std::min(cand, runs * ((runlen - 1 + unit - 1) / unit + 1));
  }
  if ((rc = check_spans(c, sp.data(), m, what, nullptr, "box"))) return rc;
  if (B > MBOX_LIST_MAX) return fail(c, DCTZHIP_E_ARG, "%s: the boxes may hit %zu tiles, more than the %zu a call lists", what, B, MBOX_LIST_MAX);
  HIPCHK(c, hipSetDevice(c->device));
  const void* side = sh ? (const void*)elems.data() : (const void*)rem_boxes.data();
  const size_t side_bytes = sh ? elems.size() * sizeof(NdBoxElems) : rem_boxes.size() * sizeof(unsigned);
  const CoarseZoom zoom = {factor, cell, (unsigned)max_cells};
  const CoarseZoom* const cz = factor ? &zoom : nullptr;
  return (st.dtype == DCTZHIP_F64) ? decompress_boxes_impl<double>(c, st, sh, k, recs.data(), side, side_bytes, (unsigned)total, B, cz)
                                   : decompress_boxes_impl<float>(c, st, sh, k, recs.data(), side, side_bytes, (unsigned)total, B, cz);
}

extern "C" int dctzhip_decompress_boxes(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                        const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf,
                                        int mode, int ndim, const size_t* dims, int k, const dctzhip_box_item* boxes) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  return decompress_boxes_call(c, "dctzhip_decompress_boxes", st, nullptr, ndim, dims, k, boxes);
}

extern "C" int dctzhip_decompress_boxes_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                           const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims, int dtype,
                                           double eb, double sf, int mode, int k, const dctzhip_box_item* boxes) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, sh.nblk * 64, dtype, eb, sf, mode};
  return decompress_boxes_call(c, "dctzhip_decompress_boxes_nd", st, &sh, ndims, dims, k, boxes);
}

// ---- the whole array at reduced resolution (include/dctz_hip.h; dctz_kernels_coarse.hip) ------------------------
// K = edge / factor coefficients kept per axis, or 0 for a factor the geometry does not have
static int coarse_k(int geom, int factor) {
  const int edge = geom == GEOM_1D ? 64 : geom == GEOM_2D ? 8 : 4;
  if (factor < 2 || factor > edge || (factor & (factor - 1))) return 0;
  return edge / factor;
}
extern "C" size_t dctzhip_coarse_len(size_t n, int factor) {
  if (!coarse_k(GEOM_1D, factor)) return 0;
  return (n + (size_t)factor - 1) / (size_t)factor;
}

// geom == GEOM_1D: sh is null, n elements in flat blocks; else the tiles of sh (n = 64 sh->nblk, no short block)
template <typename T>
static int decompress_coarse_impl(dctzhip_ctx* c, const StreamSet& st, const NdShape* sh, int factor, T* d_out) {
  hipStream_t s = c->stream;
  const size_t n = st.n;
  const int mode = st.mode, geom = !sh ? GEOM_1D : sh->nd == 2 ? GEOM_2D : GEOM_3D;
  const int k = coarse_k(geom, factor);
  const unsigned nfull = (unsigned)(n / 64);
  const int rem = (int)(n % 64);
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
  CoarseParams<T> p;
  ra_fill<T>(c, p, st, d_out);
  p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.n = (unsigned)n; p.nfull = nfull; p.ntiles = (nfull + (unsigned)TILE_BLKS - 1u) / (unsigned)TILE_BLKS;
  p.factor = (unsigned)factor;
  last_axes(sh ? sh->nd : 0, p.nb, 1u, [&](int i) { return sh->nb[i]; });
  last_axes(sh ? sh->nd : 0, p.od, 1u, [&](int i) { return (sh->d[i] + (size_t)factor - 1) / (size_t)factor; });
  if (k == 1) {
    // the DC stream alone
    if (nfull) launch_decompress_coarse_dc<T>(st.dc, d_out, nfull, (T)st.sf, s);
    SET_LAST(c, 1, "k_decompress_coarse_dc<%s>", tname<T>());
  } else {
    // a workgroup per stream tile
    if (p.ntiles) {
      int& occ = c->coarse_occ[sizeof(T) == 8][mode == DCTZHIP_QT][geom][k == 2 ? 0 : k == 4 ? 1 : k == 8 ? 2 : k == 16 ? 3 : 4];
      launch_decompress_coarse<T>(p, mode, geom, k, (int)resident_grid(c, occ, p.ntiles, [&] { return coarse_occupancy<T>(mode, geom, k); }), s);
    }
    if (geom == GEOM_1D) SET_LAST(c, 1, "k_decompress_coarse<%s, %d, %d>", tname<T>(), mode, k);
    else SET_LAST(c, 1, "k_decompress_coarse_nd<%s, %d, %d, %d>", tname<T>(), mode, geom, k);
  }
  if (rem) launch_decompress_coarse_rem<T>(p, mode, s);
  return ra_finish(c);
}

// The checks the two entry points share; n_out: elements of the output.  Not streams_given: with factor == block edge the DC
// stream alone is read and the other streams may be missing -- but for the flat short block, which is decoded in full.
static int coarse_check(dctzhip_ctx* c, const char* what, int geom, const StreamSet& st, size_t n_out, int factor, const void* d_out) {
  const int k = coarse_k(geom, factor);
  if (!k)
    return fail(c, DCTZHIP_E_ARG, "%s: factor %d is not one of %s", what, factor,
                geom == GEOM_1D ? "2, 4, 8, 16, 32, 64" : geom == GEOM_2D ? "2, 4, 8" : "2, 4");
  const bool need_ac = k > 1 || (st.n % 64) != 0;
  if (!st.dc || !d_out) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (need_ac && (!st.bin || !st.index || (st.ac_count && !st.ac))) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_out) || ((uintptr_t)st.dc & 3u)) return fail(c, DCTZHIP_E_ARG, "the output must be 16-byte aligned, DC 4-byte aligned");
  if (need_ac && (!aligned16(st.bin) || ((uintptr_t)st.ac & 3u) || ((uintptr_t)st.index & 3u)))
    return fail(c, DCTZHIP_E_ARG, "bin_index must be 16-byte aligned, AC_exact and the index 4-byte aligned");
  if (st.mode == DCTZHIP_QT && !st.qtable) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
  Span sp[5];
  size_t m = 0;
  if (need_ac) {
    tile_read_spans(sp, &m, st, 0, dctzhip_ac_index_len(st.n) - 1, 0);
    add_span(sp, &m, st.ac, (size_t)st.ac_count * sizeof(float), SPAN_READ, 0);
  } else {
    add_span(sp, &m, st.dc, (st.n + 63) / 64 * sizeof(float), SPAN_READ, 0);
  }
  add_span(sp, &m, d_out, n_out * elem_size(st.dtype), SPAN_OUT, 0);
  return check_spans(c, sp, m, what, nullptr);
}

extern "C" int dctzhip_decompress_coarse(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                         const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf,
                                         int mode, int factor, void* d_out) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  rc = coarse_check(c, "dctzhip_decompress_coarse", GEOM_1D, st, dctzhip_coarse_len(n, factor), factor, d_out);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64) ? decompress_coarse_impl<double>(c, st, nullptr, factor, (double*)d_out)
                                : decompress_coarse_impl<float>(c, st, nullptr, factor, (float*)d_out);
}

extern "C" int dctzhip_decompress_coarse_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                            const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims, int dtype,
                                            double eb, double sf, int mode, int factor, void* d_out) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const int geom = ndims == 2 ? GEOM_2D : GEOM_3D;
  size_t n_out = 1;
  if (coarse_k(geom, factor))
    for (int i = 0; i < ndims; i++) n_out *= (dims[i] + (size_t)factor - 1) / (size_t)factor;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, sh.nblk * 64, dtype, eb, sf, mode};
  rc = coarse_check(c, "dctzhip_decompress_coarse_nd", geom, st, n_out, factor, d_out);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64) ? decompress_coarse_impl<double>(c, st, &sh, factor, (double*)d_out)
                                : decompress_coarse_impl<float>(c, st, &sh, factor, (float*)d_out);
}

// ---- a box of a tiled array at reduced resolution (include/dctz_hip.h; dctz_kernels_ndcbox.hip) -----------------
// cs: the coarse array as a shape -- extents ceil(dims / factor) over the block grid of the array itself; a block owns k cells
// of it per axis.  The box is checked; [t0, t1) are its candidate stream tiles.
template <typename T>
static int decompress_coarse_box_nd_impl(dctzhip_ctx* c, const StreamSet& st, const NdShape& cs, int factor, int k, const size_t* lo,
                                         const size_t* hi, unsigned t0, unsigned t1, T* d_out) {
  hipStream_t s = c->stream;
  const int mode = st.mode, geom = cs.nd == 2 ? GEOM_2D : GEOM_3D;
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  CoarseBoxParams<T> p;
  ra_fill<T>(c, p.c, st, d_out);
  p.c.rtab = nullptr;
  p.c.n = (unsigned)(cs.nblk * 64); p.c.nfull = (unsigned)cs.nblk; p.c.ntiles = (p.c.nfull + (unsigned)TILE_BLKS - 1u) / (unsigned)TILE_BLKS;
  p.c.factor = (unsigned)factor;
  last_axes(cs.nd, p.c.od, 1u, [&](int i) { return cs.d[i]; });
  p.t0 = t0; p.t1 = t1;
  nd_box_geometry(cs, lo, hi, p.c.nb, p.lo, p.ext, &p.blocks, (unsigned)k);
  if (k == 1) {
    // the block grid is the output grid: the DC stream alone
    c->box_grid = launch_ndcoarse_box_dc<T>(st.dc, d_out, p.c.nb, p.lo, p.ext, (T)st.sf, s); c->box_tiles = 0;
    SET_LAST(c, 1, "k_ndcoarse_box_dc<%s>", tname<T>());
  } else {
    // a workgroup per candidate tile
    const unsigned tiles = t1 - t0;
    // (the kernel is small: 32 of its workgroups fit a CU, so most boxes are resident at once.  DCTZHIP_WG_PER_CU, as for the
    // big kernels, sets the number instead: the grid-stride loop on purpose, for A/B runs and tests)
    int forced = c->wg_per_cu;
    int& occ = forced ? forced : c->ndcbox_occ[sizeof(T) == 8][mode == DCTZHIP_QT][cs.nd == 3][k == 4];
    const int grid = (int)resident_grid(c, occ, tiles, [&] { return ndcbox_occupancy<T>(mode, geom, k); });
    c->box_grid = (unsigned)grid; c->box_tiles = tiles;
    launch_ndcoarse_box<T>(p, mode, geom, k, grid, s);
    SET_LAST(c, 1, "k_ndcoarse_box<%s, %d, %d, %d>", tname<T>(), mode, geom, k);
  }
  return ra_finish(c);
}

extern "C" int dctzhip_decompress_coarse_box_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                                const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims,
                                                int dtype, double eb, double sf, int mode, int factor, const size_t* lo,
                                                const size_t* hi, void* d_out) {
  static const char* const what = "dctzhip_decompress_coarse_box_nd";
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const int geom = ndims == 2 ? GEOM_2D : GEOM_3D;
  const int k = coarse_k(geom, factor);
  if (!k) return fail(c, DCTZHIP_E_ARG, "%s: factor %d is not one of %s", what, factor, geom == GEOM_2D ? "2, 4, 8" : "2, 4");
  NdShape cs = sh;
  for (int i = 0; i < ndims; i++) cs.d[i] = (sh.d[i] + (size_t)factor - 1) / (size_t)factor;
  size_t cnt = 1;
  unsigned t0 = 0, t1 = 0;
  if ((rc = nd_box_front(c, what, cs, lo, hi, &cnt, &t0, &t1, (size_t)k))) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, sh.nblk * 64, dtype, eb, sf, mode};
  if (k > 1) {
    if ((rc = streams_given(c, st, " and the output", true, d_out))) return rc;
    // what the call may read: the candidate tiles and AC_exact
    if ((rc = ra_check_spans(c, what, st, t0, t1, d_out, cnt * elem_size(dtype)))) return rc;
  } else {
    // the DC stream alone, from the first to the last block of the box
    if (!st.dc || !d_out) return fail(c, DCTZHIP_E_ARG, "null device buffer");
    if (!aligned16(d_out) || ((uintptr_t)st.dc & 3u)) return fail(c, DCTZHIP_E_ARG, "the output must be 16-byte aligned, DC 4-byte aligned");
    if (mode == DCTZHIP_QT && !qtable_host) return fail(c, DCTZHIP_E_ARG, "QT mode needs the 64-entry table");
    size_t first = 0, last = 0;
    for (int i = 0; i < ndims; i++) { first = first * sh.nb[i] + lo[i]; last = last * sh.nb[i] + (hi[i] - 1); }
    Span sp[2];
    size_t m = 0;
    add_span(sp, &m, st.dc + first, (last - first + 1) * sizeof(float), SPAN_READ, 0);
    add_span(sp, &m, d_out, cnt * elem_size(dtype), SPAN_OUT, 0);
    if ((rc = check_spans(c, sp, m, what, nullptr))) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64) ? decompress_coarse_box_nd_impl<double>(c, st, cs, factor, k, lo, hi, t0, t1, (double*)d_out)
                                : decompress_coarse_box_nd_impl<float>(c, st, cs, factor, k, lo, hi, t0, t1, (float*)d_out);
}

// ---- a list of such boxes in one call (include/dctz_hip.h; dctz_kernels_mcboxnd.hip) -----------------------------
// The list calls' host path (decompress_boxes_call) over the coarse shape, formed as the single call forms it.
extern "C" int dctzhip_decompress_coarse_boxes_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                                  const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims,
                                                  int dtype, double eb, double sf, int mode, int factor, int k,
                                                  const dctzhip_box_item* boxes) {
  static const char* const what = "dctzhip_decompress_coarse_boxes_nd";
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const int geom = ndims == 2 ? GEOM_2D : GEOM_3D;
  const int cell = coarse_k(geom, factor);
  if (!cell) return fail(c, DCTZHIP_E_ARG, "%s: factor %d is not one of %s", what, factor, geom == GEOM_2D ? "2, 4, 8" : "2, 4");
  NdShape cs = sh;
  for (int i = 0; i < ndims; i++) cs.d[i] = (sh.d[i] + (size_t)factor - 1) / (size_t)factor;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, sh.nblk * 64, dtype, eb, sf, mode};
  return decompress_boxes_call(c, what, st, &cs, ndims, dims, k, boxes, factor, cell);
}

// ---- what the summary and correction-list calls share: a whole stream set with its index, flat or tiled ----------
// streams_given, and what the call reads of the streams -- all of it -- in front of the caller's own ranges in sp.
static int streams_check(dctzhip_ctx* c, const StreamSet& st, Span* sp, size_t* m) {
  const int rc = streams_given(c, st, "");
  if (rc) return rc;
  tile_read_spans(sp, m, st, 0, dctzhip_ac_index_len(st.n) - 1, 0);
  add_span(sp, m, st.ac, (size_t)st.ac_count * sizeof(float), SPAN_READ, 0);
  return DCTZHIP_OK;
}
// The entries of a correction list over n stream positions, written (SPAN_OUT, `entries` the capacity) or read (SPAN_READ,
// `entries` the count): aligned, and their ranges behind the caller's in sp.  Whether the arrays must be given is the caller's.
static int fixlist_check(dctzhip_ctx* c, const char* what, size_t n, int dtype, const uint32_t* d_fix_start, const uint16_t* d_fix_off,
                         const void* d_fix_val, uint32_t entries, int kind, Span* sp, size_t* m) {
  const size_t es = elem_size(dtype);
  if (((uintptr_t)d_fix_off & 1u) || ((uintptr_t)d_fix_val & (es - 1)))
    return fail(c, DCTZHIP_E_ARG, "%s: fix_off must be 2-byte aligned, fix_val aligned to its elements", what);
  add_span(sp, m, d_fix_start, (dctzhip_fixup_tiles(n) + 1) * sizeof(uint32_t), kind, 0);
  add_span(sp, m, d_fix_off, (size_t)entries * sizeof(uint16_t), kind, 0);
  add_span(sp, m, d_fix_val, (size_t)entries * es, kind, 0);
  return DCTZHIP_OK;
}
// a tiled array in the last sh.nd of three axes
static void ndfix_axes(const NdShape& sh, unsigned (&nb)[3], unsigned (&d)[3]) {
  last_axes(sh.nd, nb, 1u, [&](int i) { return sh.nb[i]; });
  last_axes(sh.nd, d, 1u, [&](int i) { return sh.d[i]; });
}

// ---- tile summaries (include/dctz_hip.h; dctz_kernels_summary.hip, tiled: dctz_kernels_ndsummary.hip) -----------
extern "C" size_t dctzhip_summary_tiles(size_t n) { return (n + (size_t)TILE_ELEMS - 1) / (size_t)TILE_ELEMS; }

// sh null: st.n elements in flat blocks; else the tiles of sh (st.n = 64 sh->nblk, no short block)
template <typename T>
static int tile_summary_impl(dctzhip_ctx* c, const StreamSet& st, const NdShape* sh, const T* d_ref, dctzhip_tile_summary_t* d_tiles,
                             dctzhip_tile_summary_t* total) {
  hipStream_t s = c->stream;
  const int mode = st.mode, geom = !sh ? GEOM_1D : sh->nd == 2 ? GEOM_2D : GEOM_3D;
  const unsigned nfull = (unsigned)(st.n / 64);
  const int rem = (int)(st.n % 64);
  const size_t m = dctzhip_summary_tiles(st.n);
  const size_t fin = total ? summary_final_slots(m) : 0;
  { int rc = regrow(c, &c->sum_buf, &c->sum_cap, fin + (d_tiles ? 0 : m), sizeof(dctzhip_tile_summary_t)); if (rc) return rc; }
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  dctzhip_tile_summary_t* recs = d_tiles ? d_tiles : c->sum_buf + fin;
  const bool ref = d_ref != nullptr;
  // what the two parameter blocks share; ntiles: the stream tiles that hold a whole block (of a tiled array all m)
  auto fill = [&](auto& p) {
    ra_fill_streams<T>(c, p, st);
    p.ref = d_ref;
    p.recs = recs;
    p.n = (unsigned)st.n; p.nfull = nfull; p.ntiles = (nfull + (unsigned)TILE_BLKS - 1u) / (unsigned)TILE_BLKS;
  };
  // a workgroup per stream tile
  int& occ = c->sum_occ[sizeof(T) == 8][mode == DCTZHIP_QT][geom][ref];
  if (!sh) {
    if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
    SummaryParams<T> p;
    fill(p);
    p.rtab = reinterpret_cast<const T*>(c->rtab);
    const int grid = p.ntiles ? (int)resident_grid(c, occ, p.ntiles, [&] { return summary_occupancy<T>(mode, ref); }) : 0;
    launch_tile_summary<T>(p, mode, ref, grid, rem != 0, s);
    SET_LAST(c, 1, "%s<%s, %d, %s>", grid ? "k_tile_summary" : "k_tile_summary_rem", tname<T>(), mode, bname(ref));
  } else {
    NdSummaryParams<T> p;
    fill(p);
    ndfix_axes(*sh, p.nb, p.d);
    const int grid = (int)resident_grid(c, occ, p.ntiles, [&] { return ndsummary_occupancy<T>(mode, geom, ref); });
    launch_tile_summary_nd<T>(p, mode, geom, ref, grid, s);
    SET_LAST(c, 1, "k_ndsummary<%s, %d, %d, %s>", tname<T>(), mode, geom, bname(ref));
  }
  dctzhip_tile_summary_t* ht = reinterpret_cast<dctzhip_tile_summary_t*>(c->h_pin + PIN_STATS);
  static_assert(sizeof(dctzhip_tile_summary_t) == 64 && PIN_CTL - PIN_STATS >= sizeof(dctzhip_tile_summary_t), "the total fits the pinned statistics slot");
  if (total) {
    const dctzhip_tile_summary_t* dt = launch_tile_summary_final(recs, m, c->sum_buf, s);
    HIPCHK(c, hipMemcpyAsync(ht, dt, sizeof(*ht), hipMemcpyDeviceToHost, s));
  }
  const int rc = ra_finish(c);
  if (rc == DCTZHIP_OK && total) *total = *ht;
  return rc;
}

// what the two entry points share once the geometry is known; n_ref: the elements of the original
static int tile_summary_call(dctzhip_ctx* c, const char* what, const StreamSet& st, const NdShape* sh, size_t n_ref, const void* d_ref,
                             dctzhip_tile_summary_t* d_tiles, dctzhip_tile_summary_t* total) {
  if (!d_tiles && !total) return fail(c, DCTZHIP_E_ARG, "%s: at least one of d_tiles and total must be given", what);
  if ((uintptr_t)d_tiles & 7u) return fail(c, DCTZHIP_E_ARG, "%s: the records must be 8-byte aligned", what);
  Span sp[6];
  size_t m = 0;
  int rc = streams_check(c, st, sp, &m);
  if (rc) return rc;
  add_span(sp, &m, d_ref, n_ref * elem_size(st.dtype), SPAN_READ, 0);
  add_span(sp, &m, d_tiles, dctzhip_summary_tiles(st.n) * sizeof(dctzhip_tile_summary_t), SPAN_OUT, 0);
  rc = check_spans(c, sp, m, what, nullptr);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (st.dtype == DCTZHIP_F64) ? tile_summary_impl<double>(c, st, sh, (const double*)d_ref, d_tiles, total)
                                   : tile_summary_impl<float>(c, st, sh, (const float*)d_ref, d_tiles, total);
}

extern "C" int dctzhip_tile_summary(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                    const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf, int mode,
                                    const void* d_ref, dctzhip_tile_summary_t* d_tiles, dctzhip_tile_summary_t* total) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  if (!aligned16(d_ref)) return fail(c, DCTZHIP_E_ARG, "dctzhip_tile_summary: the original must be 16-byte aligned");
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  return tile_summary_call(c, "dctzhip_tile_summary", st, nullptr, n, d_ref, d_tiles, total);
}

extern "C" int dctzhip_tile_summary_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                       const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims, int dtype, double eb,
                                       double sf, int mode, const void* d_ref, dctzhip_tile_summary_t* d_tiles, dctzhip_tile_summary_t* total) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const size_t n_lin = sh.nblk * 64, n_orig = sh.d[0] * sh.d[1] * sh.d[2];
  // (the original is read element by element at its own coordinates: the rows of a ragged array are not 16-byte aligned anyway)
  if ((uintptr_t)d_ref & (elem_size(dtype) - 1)) return fail(c, DCTZHIP_E_ARG, "dctzhip_tile_summary_nd: the original must be aligned to its elements");
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n_lin, dtype, eb, sf, mode};
  return tile_summary_call(c, "dctzhip_tile_summary_nd", st, &sh, n_orig, d_ref, d_tiles, total);
}

// ---- correction list for a point-wise bound (include/dctz_hip.h; dctz_kernels_fixup.hip, tiled: dctz_kernels_ndfix.hip) ----
extern "C" size_t dctzhip_fixup_tiles(size_t n) { return (n + (size_t)TILE_ELEMS - 1) / (size_t)TILE_ELEMS; }

// sh as for tile_summary_impl; what: the entry point, for the report of a list that does not fit
template <typename T>
static int fixup_build_impl(dctzhip_ctx* c, const char* what, const StreamSet& st, const NdShape* sh, const T* d_ref, double bound,
                            uint32_t* d_fix_start, uint16_t* d_fix_off, T* d_fix_val, uint32_t capacity, uint32_t* count) {
  hipStream_t s = c->stream;
  const int mode = st.mode, geom = !sh ? GEOM_1D : sh->nd == 2 ? GEOM_2D : GEOM_3D;
  const unsigned nfull = (unsigned)(st.n / 64);
  const int rem = (int)(st.n % 64);
  const size_t m = dctzhip_fixup_tiles(st.n);
  { int rc = regrow(c, &c->fix_mask, &c->fix_mask_cap, (st.n + 63) / 64, sizeof(unsigned long long)); if (rc) return rc; }
  { int rc = regrow(c, &c->fix_cnt, &c->fix_cnt_cap, m + fixup_scan_slots(m), sizeof(unsigned)); if (rc) return rc; }
  { int rc = ra_begin<T>(c, mode, st.qtable); if (rc) return rc; }
  // what the two parameter blocks share; q: where a block keeps the streams.  ntiles as for tile_summary_impl
  auto fill = [&](auto& p, auto& q) {
    ra_fill_streams<T>(c, q, st);
    q.ref = d_ref;
    q.n = (unsigned)st.n; q.nfull = nfull; q.ntiles = (nfull + (unsigned)TILE_BLKS - 1u) / (unsigned)TILE_BLKS;
    p.bound = (T)bound;
    p.mask = c->fix_mask;
    p.tile_cnt = c->fix_cnt;
  };
  // a workgroup per stream tile
  int& occ = c->fix_occ[sizeof(T) == 8][mode == DCTZHIP_QT][geom];
  if (!sh) {
    if (rem) { int rc = upload_rtab<T>(c, rem); if (rc) return rc; }
    FixupParams<T> p;
    fill(p, p.s);
    p.s.rtab = reinterpret_cast<const T*>(c->rtab);
    p.s.recs = nullptr;
    const int grid = p.s.ntiles ? (int)resident_grid(c, occ, p.s.ntiles, [&] { return fixup_occupancy<T>(mode); }) : 0;
    launch_fixup_mark<T>(p, mode, grid, rem != 0, s);
    SET_LAST(c, 1, "%s<%s, %d>", grid ? "k_fixup_mark" : "k_fixup_mark_rem", tname<T>(), mode);
  } else {
    NdFixParams<T> p;
    fill(p, p);
    ndfix_axes(*sh, p.nb, p.d);
    const int grid = (int)resident_grid(c, occ, p.ntiles, [&] { return ndfix_occupancy<T>(mode, geom); });
    launch_ndfix_mark<T>(p, mode, geom, grid, s);
    SET_LAST(c, 1, "k_ndfix_mark<%s, %d, %d>", tname<T>(), mode, geom);
  }
  launch_fixup_scan(c->fix_cnt, m, d_fix_start, c->fix_cnt + m, c->ctl, s);
  if (d_fix_off) {
    // behind the scan in stream order; the kernel itself stands back if the list does not fit or a tile was refused
    auto fill_emit = [&](auto& e) {
      e.mask = c->fix_mask; e.fix_start = d_fix_start; e.ref = d_ref; e.fix_off = d_fix_off; e.fix_val = d_fix_val; e.ctl = c->ctl;
      e.capacity = capacity;
    };
    const int g = (int)std::min<size_t>(m, (size_t)c->num_cu * 32);                 // (a few registers, no LDS: eight waves per SIMD)
    if (!sh) {
      FixupEmitParams<T> e;
      fill_emit(e);
      e.n = (unsigned)st.n;
      launch_fixup_emit<T>(e, g, s);
    } else {
      NdFixEmitParams<T> e;
      fill_emit(e);
      e.nblk = nfull; e.ntiles = (unsigned)m;
      ndfix_axes(*sh, e.nb, e.d);
      launch_ndfix_emit<T>(e, geom, g, s);
    }
  }
  unsigned total = 0;
  const int rc = ra_finish(c, &total);                 // (the control block's counter was used: the next call clears the block)
  if (rc) return rc;
  *count = total;
  if (d_fix_off && total > capacity) return fail(c, DCTZHIP_E_SPACE, "%s: %u entries do not fit the capacity of %u", what, total, capacity);
  return DCTZHIP_OK;
}

// what the two entry points share once the geometry is known; n_ref: the elements of the original
static int fixup_build_call(dctzhip_ctx* c, const char* what, const StreamSet& st, const NdShape* sh, size_t n_ref, const void* d_ref,
                            double bound, uint32_t* d_fix_start, uint16_t* d_fix_off, void* d_fix_val, uint32_t capacity, uint32_t* count) {
  if (!d_ref || !count) return fail(c, DCTZHIP_E_ARG, "%s: the original and count must be given", what);
  if (!(bound >= 0.0) || std::isinf(bound)) return fail(c, DCTZHIP_E_ARG, "%s: the bound must be finite and >= 0", what);
  if (!aligned16(d_ref)) return fail(c, DCTZHIP_E_ARG, "%s: the original must be 16-byte aligned", what);
  if (!d_fix_start || ((uintptr_t)d_fix_start & 3u)) return fail(c, DCTZHIP_E_ARG, "%s: fix_start must be given, 4-byte aligned", what);
  if ((d_fix_off == nullptr) != (d_fix_val == nullptr)) return fail(c, DCTZHIP_E_ARG, "%s: fix_off and fix_val must both be given or both be NULL", what);
  Span sp[8];
  size_t m = 0;
  int rc = streams_check(c, st, sp, &m);
  if (rc) return rc;
  add_span(sp, &m, d_ref, n_ref * elem_size(st.dtype), SPAN_READ, 0);
  rc = fixlist_check(c, what, st.n, st.dtype, d_fix_start, d_fix_off, d_fix_val, capacity, SPAN_OUT, sp, &m);
  if (rc) return rc;
  rc = check_spans(c, sp, m, what, nullptr);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (st.dtype == DCTZHIP_F64)
             ? fixup_build_impl<double>(c, what, st, sh, (const double*)d_ref, bound, d_fix_start, d_fix_off, (double*)d_fix_val, capacity, count)
             : fixup_build_impl<float>(c, what, st, sh, (const float*)d_ref, bound, d_fix_start, d_fix_off, (float*)d_fix_val, capacity, count);
}

extern "C" int dctzhip_fixup_build(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                   const uint32_t* d_index, const void* qtable_host, size_t n, int dtype, double eb, double sf, int mode,
                                   const void* d_ref, double bound, uint32_t* d_fix_start, uint16_t* d_fix_off, void* d_fix_val,
                                   uint32_t capacity, uint32_t* count) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n, dtype, eb, sf, mode};
  return fixup_build_call(c, "dctzhip_fixup_build", st, nullptr, n, d_ref, bound, d_fix_start, d_fix_off, d_fix_val, capacity, count);
}

extern "C" int dctzhip_fixup_build_nd(dctzhip_ctx* c, const void* d_bin, const float* d_dc, const float* d_ac, uint32_t ac_count,
                                      const uint32_t* d_index, const void* qtable_host, int ndims, const size_t* dims, int dtype, double eb,
                                      double sf, int mode, const void* d_ref, double bound, uint32_t* d_fix_start, uint16_t* d_fix_off,
                                      void* d_fix_val, uint32_t capacity, uint32_t* count) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const size_t n_lin = sh.nblk * 64, n_orig = sh.d[0] * sh.d[1] * sh.d[2];
  const StreamSet st = {(const uint8_t*)d_bin, d_dc, d_ac, ac_count, d_index, qtable_host, n_lin, dtype, eb, sf, mode};
  return fixup_build_call(c, "dctzhip_fixup_build_nd", st, &sh, n_orig, d_ref, bound, d_fix_start, d_fix_off, d_fix_val, capacity, count);
}

// sh null: the box of the flat n-element array, its stream tiles [t0, t1) of 4096 elements; else the box [lo, hi) of the
// tiled array, the stream tiles [t0, t1) of 64 blocks (n = 64 sh->nblk)
template <typename T>
static int fixup_apply_impl(dctzhip_ctx* c, const uint32_t* d_fix_start, const uint16_t* d_fix_off, const T* d_fix_val, uint32_t count, size_t n,
                            const NdShape* sh, const BoxGeo* box, const size_t* lo, const size_t* hi, unsigned t0, unsigned t1, T* d_out) {
  hipStream_t s = c->stream;
  { int rc = ra_begin<T>(c, DCTZHIP_EC, nullptr); if (rc) return rc; }
  auto fill = [&](auto& p) {
    p.fix_start = d_fix_start; p.fix_off = d_fix_off; p.fix_val = d_fix_val; p.out = d_out; p.ctl = c->ctl;
    p.count = count; p.t0 = t0; p.t1 = t1;
  };
  const unsigned tiles = t1 - t0, resident = (unsigned)c->num_cu * 32u;              // (a few registers, no LDS: eight waves per SIMD)
  const int grid = (int)(tiles < resident ? tiles : resident);
  if (!sh) {
    FixupApplyParams<T> p;
    fill(p);
    p.n = (unsigned)n;
    p.box = *box;
    launch_fixup_apply<T>(p, grid, s);
    SET_LAST(c, 1, "k_fixup_apply<%s>", tname<T>());
  } else {
    const int geom = sh->nd == 2 ? GEOM_2D : GEOM_3D;
    NdFixApplyParams<T> p;
    fill(p);
    p.nblk = (unsigned)sh->nblk; p.ntiles = (unsigned)dctzhip_fixup_tiles(n);
    ndfix_axes(*sh, p.nb, p.d);
    last_axes(sh->nd, p.lo, 0u, [&](int i) { return lo[i]; });
    last_axes(sh->nd, p.ext, 1u, [&](int i) { return hi[i] - lo[i]; });
    launch_ndfix_apply<T>(p, geom, grid, s);
    SET_LAST(c, 1, "k_ndfix_apply<%s, %d>", tname<T>(), geom);
  }
  return ra_finish(c);
}

// what the two entry points share once the box is known to lie in the array; n: the stream positions, cnt: the elements of the box
static int fixup_apply_call(dctzhip_ctx* c, const char* what, const uint32_t* d_fix_start, const uint16_t* d_fix_off, const void* d_fix_val,
                            uint32_t count, size_t n, int dtype, const NdShape* sh, const BoxGeo* box, const size_t* lo, const size_t* hi,
                            unsigned t0, unsigned t1, size_t cnt, void* d_out) {
  const size_t es = elem_size(dtype);
  if (!d_fix_start || !d_out || ((uintptr_t)d_fix_start & 3u) || ((uintptr_t)d_out & (es - 1)))
    return fail(c, DCTZHIP_E_ARG, "%s: fix_start and the output must be given, 4-byte / element aligned", what);
  if (count && (!d_fix_off || !d_fix_val)) return fail(c, DCTZHIP_E_ARG, "%s: null fix_off or fix_val", what);
  Span sp[4];
  size_t m = 0;
  int rc = fixlist_check(c, what, n, dtype, d_fix_start, d_fix_off, d_fix_val, count, SPAN_READ, sp, &m);
  if (rc) return rc;
  add_span(sp, &m, d_out, cnt * es, SPAN_OUT, 0);
  rc = check_spans(c, sp, m, what, nullptr);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return (dtype == DCTZHIP_F64)
             ? fixup_apply_impl<double>(c, d_fix_start, d_fix_off, (const double*)d_fix_val, count, n, sh, box, lo, hi, t0, t1, (double*)d_out)
             : fixup_apply_impl<float>(c, d_fix_start, d_fix_off, (const float*)d_fix_val, count, n, sh, box, lo, hi, t0, t1, (float*)d_out);
}

extern "C" int dctzhip_fixup_apply(dctzhip_ctx* c, const uint32_t* d_fix_start, const uint16_t* d_fix_off, const void* d_fix_val, uint32_t count,
                                   size_t n, int dtype, int ndim, const size_t* dims, const size_t* lo, const size_t* hi, void* d_out) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  size_t cnt = 1, first = 0, last = 0;
  rc = box_front(c, "dctzhip_fixup_apply", n, ndim, dims, lo, hi, &cnt, &first, &last);
  if (rc) return rc;
  if (count > n) return fail(c, DCTZHIP_E_ARG, "dctzhip_fixup_apply: count %u exceeds n = %zu", count, n);
  const BoxGeo box = canonical_box(ndim, dims, lo, hi);
  return fixup_apply_call(c, "dctzhip_fixup_apply", d_fix_start, d_fix_off, d_fix_val, count, n, dtype, nullptr, &box, nullptr, nullptr,
                          (unsigned)(first / TILE_ELEMS), (unsigned)(last / TILE_ELEMS + 1), cnt, d_out);
}

extern "C" int dctzhip_fixup_apply_nd(dctzhip_ctx* c, const uint32_t* d_fix_start, const uint16_t* d_fix_off, const void* d_fix_val,
                                      uint32_t count, int ndims, const size_t* dims, int dtype, const size_t* lo, const size_t* hi,
                                      void* d_out) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, DCTZHIP_EC, &sh);
  if (rc) return rc;
  const size_t n_lin = sh.nblk * 64, n_orig = sh.d[0] * sh.d[1] * sh.d[2];
  size_t cnt = 1;
  unsigned t0 = 0, t1 = 0;
  if ((rc = nd_box_front(c, "dctzhip_fixup_apply_nd", sh, lo, hi, &cnt, &t0, &t1))) return rc;
  if (count > n_orig) return fail(c, DCTZHIP_E_ARG, "dctzhip_fixup_apply_nd: count %u exceeds the array's %zu elements", count, n_orig);
  return fixup_apply_call(c, "dctzhip_fixup_apply_nd", d_fix_start, d_fix_off, d_fix_val, count, n_lin, dtype, &sh, nullptr, lo, hi, t0, t1, cnt,
                          d_out);
}

// ---- missing values: a mask beside the streams (include/dctz_hip.h; dctz_kernels_mask.hip) ----------------------
extern "C" size_t dctzhip_mask_words(size_t n) { return (n + 63) / 64; }

static int check_missing(dctzhip_ctx* c, const char* what, const dctzhip_missing* miss) {
  const unsigned all = DCTZHIP_MISS_NAN | DCTZHIP_MISS_INF | DCTZHIP_MISS_VALUE | DCTZHIP_MISS_ABS_GE;
  if (!miss) return fail(c, DCTZHIP_E_ARG, "%s: the missing-value rule must be given", what);
  if (miss->flags == 0 || (miss->flags & ~all)) return fail(c, DCTZHIP_E_ARG, "%s: flags 0x%x select no test or an unknown one", what, miss->flags);
  if ((miss->flags & DCTZHIP_MISS_VALUE) && std::isnan(miss->value))
    return fail(c, DCTZHIP_E_ARG, "%s: a NaN value matches nothing; use DCTZHIP_MISS_NAN", what);
  if ((miss->flags & DCTZHIP_MISS_ABS_GE) && !(miss->limit > 0.0 && std::isfinite(miss->limit)))
    return fail(c, DCTZHIP_E_ARG, "%s: the limit must be finite and > 0", what);
  return DCTZHIP_OK;
}

// The arguments are checked.  sh null: n elements in flat blocks (dctz_kernels_mask.hip); else the tiles of sh, n = prod dims
// <= 64 nblk <= INT_MAX (nd_shape; dctz_kernels_ndmask.hip).  The count is the control block's counter, read back with the
// error word.
template <typename T>
static int mask_build_impl(dctzhip_ctx* c, const T* d_in, size_t n, const NdShape* sh, const dctzhip_missing* miss, uint64_t* d_mask,
                           T* d_filled, uint64_t* count) {
  c->ctl_dirty = 1;                                    // the kernel ADDS to the control block's counter: cleared in stream order, always
  { int rc = ra_begin<T>(c, DCTZHIP_EC, nullptr); if (rc) return rc; }
  // what the two parameter blocks share
  auto fill = [&](auto& p) {
    p.in = d_in; p.out = d_filled; p.mask32 = reinterpret_cast<unsigned*>(d_mask); p.ctl = c->ctl;
    p.flags = miss->flags;
    p.value = (T)miss->value; p.limit = (T)miss->limit;
  };
  // a wave trip is 1 KiB of the array, MASK_TRIPS of them at a time; eight waves per SIMD (a few registers, no LDS), persistent beyond that
  auto grid = [&](size_t trips) {
    const size_t per_wg = (size_t)(MASK_WG / 64) * MASK_TRIPS, wgs = (trips + per_wg - 1) / per_wg;
    return (int)std::min<size_t>(wgs, (size_t)c->num_cu * 8);
  };
  if (!sh) {
    MaskFillParams<T> p;
    fill(p);
    p.n = (unsigned)n;
    launch_mask_fill<T>(p, grid((n * sizeof(T) + 1023) / 1024), c->stream);
    SET_LAST(c, 1, "k_mask_fill<%s>", tname<T>());
  } else {
    constexpr size_t E = 16 / sizeof(T);
    const size_t width = (sh->nd == 2 ? 8 : 4) * E;                                      // elements of a trip row
    NdMaskFillParams<T> p;
    fill(p);
    p.dz = sh->nd == 3 ? (unsigned)sh->d[0] : 1u; p.dy = (unsigned)sh->d[sh->nd - 2]; p.dx = (unsigned)sh->d[sh->nd - 1];
    p.nby = (unsigned)sh->nb[sh->nd - 2];
    p.ntx = (unsigned)((sh->nb[sh->nd - 1] + E - 1) / E);
    const size_t trips = (sh->nd == 3 ? sh->nb[0] : 1) * p.nby * (size_t)p.ntx;          // <= nblk
    p.trips = (unsigned)trips;
    p.pitch16 = sh->d[sh->nd - 1] * sizeof(T) % 16 == 0;
    p.plain = sh->d[sh->nd - 1] % width == 0;
    // plain: the trip rows are the bytes of the bits below n, all stored; what the last word has beyond n is cleared here.
    // Else every row is ORed into a cleared mask.
    const size_t words = dctzhip_mask_words(n);
    if (!p.plain) HIPCHK(c, hipMemsetAsync(d_mask, 0, words * sizeof(uint64_t), c->stream));
    else if (n % 64) HIPCHK(c, hipMemsetAsync(d_mask + words - 1, 0, sizeof(uint64_t), c->stream));
    launch_ndmask_fill<T>(p, sh->nd == 2 ? GEOM_2D : GEOM_3D, grid(trips), c->stream);
    SET_LAST(c, 1, "k_ndmask_fill<%s, %d>", tname<T>(), sh->nd == 2 ? GEOM_2D : GEOM_3D);
  }
  unsigned total = 0;
  const int rc = ra_finish(c, &total);                 // (the control block's counter was used: the next call clears the block)
  if (rc) return rc;
  *count = total;
  return DCTZHIP_OK;
}
// the only dtype dispatch of the build
static int mask_build_call(dctzhip_ctx* c, const void* d_in, size_t n, const NdShape* sh, int dtype, const dctzhip_missing* miss, uint64_t* d_mask,
                           void* d_filled, uint64_t* count) {
  return (dtype == DCTZHIP_F64) ? mask_build_impl<double>(c, (const double*)d_in, n, sh, miss, d_mask, (double*)d_filled, count)
                                : mask_build_impl<float>(c, (const float*)d_in, n, sh, miss, d_mask, (float*)d_filled, count);
}
// The tail the two masked compress calls share in front of their compress: the filled copy is the context's where the caller
// gives none (*d_filled is set to it), then the build.
static int masked_build(dctzhip_ctx* c, const void* d_in, size_t n, const NdShape* sh, int dtype, const dctzhip_missing* miss, uint64_t* d_mask,
                        void** d_filled, uint64_t* count) {
  if (!*d_filled) {
    const int rc = regrow(c, &c->mask_filled, &c->mask_filled_cap, n * elem_size(dtype), 1);
    if (rc) return rc;
    *d_filled = c->mask_filled;
  }
  return mask_build_call(c, d_in, n, sh, dtype, miss, d_mask, *d_filled, count);
}

// The refusals the two builds share, and the tiled masked compress with them, behind the geometry, dtype and NULL checks of
// each: the rule, alignment, and the buffers against each other.  n: the array's elements; d_filled: NULL, d_in itself (where
// in_place_ok) or disjoint; sp[0 .. m) holds the spans of the caller's other buffers and has room for three more.
static int check_mask(dctzhip_ctx* c, const char* what, const void* d_in, size_t n, int dtype, const dctzhip_missing* miss,
                      const uint64_t* d_mask, const void* d_filled, bool in_place_ok, Span* sp, size_t m) {
  int rc = check_missing(c, what, miss);
  if (rc) return rc;
  if (!aligned16(d_in) || !aligned16(d_filled) || ((uintptr_t)d_mask & 7u))
    return fail(c, DCTZHIP_E_ARG, "%s: the arrays must be 16-byte aligned, the mask 8-byte aligned", what);
  const size_t es = elem_size(dtype);
  const bool in_place = in_place_ok && d_filled == d_in;
  add_span(sp, &m, d_in, n * es, in_place ? SPAN_IN_PLACE : SPAN_READ, 0);
  if (!in_place) add_span(sp, &m, d_filled, n * es, SPAN_OUT, 0);
  add_span(sp, &m, d_mask, dctzhip_mask_words(n) * sizeof(uint64_t), SPAN_OUT, 0);
  return check_spans(c, sp, m, what, nullptr);
}

extern "C" int dctzhip_mask_build(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, const dctzhip_missing* miss, uint64_t* d_mask,
                                  void* d_filled, uint64_t* count) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_in || !d_mask || !count) return fail(c, DCTZHIP_E_ARG, "dctzhip_mask_build: the array, the mask and count must be given");
  Span sp[3];
  rc = check_mask(c, "dctzhip_mask_build", d_in, n, dtype, miss, d_mask, d_filled, true, sp, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return mask_build_call(c, d_in, n, nullptr, dtype, miss, d_mask, d_filled, count);
}

extern "C" int dctzhip_compress_masked(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, double eb, int mode, const dctzhip_missing* miss,
                                       void* d_bin, float* d_dc, float* d_ac, uint64_t* d_mask, void* d_filled, dctzhip_cinfo* info,
                                       uint64_t* count) {
  int rc = check_common(c, n, dtype, mode);
  if (rc) return rc;
  if (!d_in || !d_bin || !d_dc || !d_ac || !d_mask || !count) return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_masked: null buffer or count");
  rc = check_missing(c, "dctzhip_compress_masked", miss);
  if (rc) return rc;
  if (!aligned16(d_in) || !aligned16(d_bin) || !aligned16(d_dc) || !aligned16(d_ac) || !aligned16(d_filled) || ((uintptr_t)d_mask & 7u))
    return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_masked: device buffers must be 16-byte aligned, the mask 8-byte aligned");
  if (eb < 1E-6) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  {
    Span sp[8];
    size_t m = 0;
    compress_spans(sp, &m, 0, d_in, n, dtype, d_bin, d_dc, d_ac, nullptr, nullptr);
    add_span(sp, &m, d_filled, n * elem_size(dtype), SPAN_OUT, 0);      // (d_in itself included: d_in is not modified)
    add_span(sp, &m, d_mask, dctzhip_mask_words(n) * sizeof(uint64_t), SPAN_OUT, 0);
    rc = check_spans(c, sp, m, "dctzhip_compress_masked", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = masked_build(c, d_in, n, nullptr, dtype, miss, d_mask, &d_filled, count))) return rc;
  return dctzhip_compress(c, d_filled, n, dtype, eb, mode, d_bin, d_dc, d_ac, nullptr, nullptr, info);
}

// The tiled twins.
extern "C" int dctzhip_mask_build_nd(dctzhip_ctx* c, const void* d_in, int ndims, const size_t* dims, int dtype, const dctzhip_missing* miss,
                                     uint64_t* d_mask, void* d_filled, uint64_t* count) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, DCTZHIP_EC, &sh);
  if (rc) return rc;
  if (!d_in || !d_mask || !count) return fail(c, DCTZHIP_E_ARG, "dctzhip_mask_build_nd: the array, the mask and count must be given");
  const size_t n = sh.d[0] * sh.d[1] * sh.d[2];
  Span sp[3];
  rc = check_mask(c, "dctzhip_mask_build_nd", d_in, n, dtype, miss, d_mask, d_filled, true, sp, 0);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return mask_build_call(c, d_in, n, &sh, dtype, miss, d_mask, d_filled, count);
}

extern "C" int dctzhip_compress_masked_nd(dctzhip_ctx* c, const void* d_in, int ndims, const size_t* dims, int dtype, double eb, int mode,
                                          const dctzhip_missing* miss, void* d_bin, float* d_dc, float* d_ac, uint64_t* d_mask,
                                          void* d_filled, dctzhip_cinfo* info, uint64_t* count) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, mode, &sh);
  if (rc) return rc;
  const size_t n_lin = sh.nblk * 64, n = sh.d[0] * sh.d[1] * sh.d[2];
  if (!d_in || !d_bin || !d_dc || !d_ac || !d_mask || !count) return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_masked_nd: null buffer or count");
  if (!aligned16(d_bin) || !aligned16(d_dc) || !aligned16(d_ac))
    return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_masked_nd: device buffers must be 16-byte aligned");
  if (eb < 1E-6) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  Span sp[6];
  size_t m = 0;
  add_span(sp, &m, d_bin, n_lin, SPAN_OUT, 0);
  add_span(sp, &m, d_dc, sh.nblk * sizeof(float), SPAN_OUT, 0);
  add_span(sp, &m, d_ac, n_lin * sizeof(float), SPAN_OUT, 0);
  rc = check_mask(c, "dctzhip_compress_masked_nd", d_in, n, dtype, miss, d_mask, d_filled, false, sp, m);   // (d_in is not modified)
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = masked_build(c, d_in, n, &sh, dtype, miss, d_mask, &d_filled, count))) return rc;
  return dctzhip_compress_nd(c, d_filled, ndims, dims, dtype, eb, mode, d_bin, d_dc, d_ac, nullptr, info);
}

template <typename T>
static int mask_apply_impl(dctzhip_ctx* c, const uint64_t* d_mask, double fill, const BoxGeo& box, size_t cnt, size_t first, T* d_out) {
  MaskApplyParams<T> p;
  p.mask32 = reinterpret_cast<const unsigned*>(d_mask); p.out = d_out; p.fill = (T)fill;
  p.cnt = (unsigned)cnt; p.first = (unsigned)first;
  p.one_run = box.ext[0] == 1u && box.ext[1] == 1u && box.ext[2] == 1u;
  p.box = box;
  const size_t wgs = (cnt + MASK_WG - 1) / MASK_WG;
  launch_mask_apply<T>(p, (int)std::min<size_t>(wgs, (size_t)c->num_cu * 8), c->stream);
  SET_LAST(c, 1, "k_mask_apply<%s>", tname<T>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

extern "C" int dctzhip_mask_apply(dctzhip_ctx* c, const uint64_t* d_mask, size_t n, int dtype, double fill, int ndim, const size_t* dims,
                                  const size_t* lo, const size_t* hi, void* d_out) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  size_t cnt = 1, first = 0, last = 0;
  rc = box_front(c, "dctzhip_mask_apply", n, ndim, dims, lo, hi, &cnt, &first, &last);
  if (rc) return rc;
  const size_t es = elem_size(dtype);
  if (!d_mask || !d_out || ((uintptr_t)d_mask & 7u) || ((uintptr_t)d_out & (es - 1)))
    return fail(c, DCTZHIP_E_ARG, "dctzhip_mask_apply: the mask and the output must be given, 8-byte / element aligned");
  {
    Span sp[2];
    size_t m = 0;
    add_span(sp, &m, d_mask + first / 64, (last / 64 - first / 64 + 1) * sizeof(uint64_t), SPAN_READ, 0);
    add_span(sp, &m, d_out, cnt * es, SPAN_OUT, 0);
    rc = check_spans(c, sp, m, "dctzhip_mask_apply", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const BoxGeo box = canonical_box(ndim, dims, lo, hi);
  return (dtype == DCTZHIP_F64) ? mask_apply_impl<double>(c, d_mask, fill, box, cnt, first, (double*)d_out)
                                : mask_apply_impl<float>(c, d_mask, fill, box, cnt, first, (float*)d_out);
}

extern "C" int dctzhip_dct_blocks(dctzhip_ctx* c, const void* d_in, void* d_out, size_t n, int dtype, int inverse) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_in || !d_out) return fail(c, DCTZHIP_E_ARG, "null device buffer");
  if (!aligned16(d_in) || !aligned16(d_out)) return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  const int rem = (int)(n % 64);
  if (dtype == DCTZHIP_F64) {
    if (rem) { rc = upload_rtab<double>(c, rem); if (rc) return rc; }
    launch_dct_blocks<double>((const double*)d_in, (double*)d_out, c->tab_f64, (const double*)c->rtab, n, inverse != 0,
                              c->num_cu * 4, c->stream);
  } else {
    if (rem) { rc = upload_rtab<float>(c, rem); if (rc) return rc; }
    launch_dct_blocks<float>((const float*)d_in, (float*)d_out, c->tab_f32, (const float*)c->rtab, n, inverse != 0,
                             c->num_cu * 4, c->stream);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

// calc_psnr's reductions (util.c:54-104) on device-resident arrays: out = {min(x), max(x), max |x - r|, sum (x - r)^2}
extern "C" int dctzhip_psnr_terms(dctzhip_ctx* c, const void* d_x, const void* d_r, size_t n, int dtype, double out[4]) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  if (!d_x || !d_r || !out) return fail(c, DCTZHIP_E_ARG, "null buffer");
  HIPCHK(c, hipSetDevice(c->device));
  int grid = (int)((n + SWG * 8 - 1) / (SWG * 8));
  if (grid < 1) grid = 1;
  if (grid > 3 * PART_SLOTS / 4) grid = 3 * PART_SLOTS / 4;       // 4 doubles per partial in the 3-per-slot array
  if (dtype == DCTZHIP_F64) launch_psnr<double>((const double*)d_x, (const double*)d_r, n, c->part, grid, c->stats_out, c->stream);
  else launch_psnr<float>((const float*)d_x, (const float*)d_r, n, c->part, grid, c->stats_out, c->stream);
  HIPCHK(c, hipGetLastError());
  double* hs = reinterpret_cast<double*>(c->h_pin + PIN_STATS);
  HIPCHK(c, hipMemcpyAsync(hs, c->stats_out, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 4; i++) out[i] = hs[i];
  return DCTZHIP_OK;
}

// ---- rate-distortion probe and target-PSNR compression (include/dctz_hip.h; dctz_kernels_rd.hip) ----------------------
// calc_psnr (util.c:54-104): 20 log10(range / rmse), rmse = sqrt(sse / N)
static double psnr_of(double lo, double hi, double sse, size_t n) { return 20.0 * log10((hi - lo) / sqrt(sse / (double)(int)n)); }

// sh == NULL: n elements in flat blocks.  Else the array of sh (n = its elements) in 8 x 8 / 4 x 4 x 4 tiles, read in place.
template <typename T>
static int rd_probe_impl(dctzhip_ctx* c, const T* d_in, size_t n, const NdShape* sh, int k, const double* ebs, dctzhip_rd_point* pts,
                         double range[2]) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  hipStream_t s = c->stream;
  double mx, mn, sum;
  int rc = stats_impl<T>(c, d_in, n, &mx, &mn, &sum);          // calc_data_stat: only sf is needed (util.c:29)
  if (rc) return rc;
  const unsigned nfull = sh ? (unsigned)sh->nblk : (unsigned)(n / 64);
  const int rem = sh ? 0 : (int)(n % 64);
  const unsigned ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  constexpr unsigned NW = RD_WG / 64;
  // one workgroup per CU (fp64: one wave per SIMD, the kernel's register budget) / two (fp32); fewer for small arrays
  unsigned grid = (unsigned)c->num_cu * (sizeof(T) == 8 ? 1u : 2u);
  if (grid > (ntiles + NW - 1) / NW) grid = (ntiles + NW - 1) / NW;
  // a tiled array: the blocks with padded places (the last tile of every ragged axis), a wave per 64 of them
  NdRdParams<T> q;
  memset(&q, 0, sizeof(q));
  unsigned edge_grid = 0;
  if (sh) {
    const size_t edge = sh->nd == 2 ? 8 : 4;
    size_t whole = 1;
    for (int i = 0; i < 3; i++) { q.d[i] = 1u; q.nb[i] = 1u; }
    for (int i = 0; i < sh->nd; i++) {
      const int a = 3 - sh->nd + i;
      q.d[a] = (unsigned)sh->d[i]; q.nb[a] = (unsigned)sh->nb[i]; q.rag[a] = sh->d[i] % edge ? 1u : 0u;
      whole *= sh->nb[i] - q.rag[a];
    }
    q.vec = sh->d[sh->nd - 1] % Traits<T>::EPV == 0 ? 1u : 0u;
    q.nedge = (unsigned)(sh->nblk - whole);
    edge_grid = (q.nedge + TILE_BLKS - 1) / TILE_BLKS;
    if (edge_grid > (unsigned)c->num_cu * 4u) edge_grid = (unsigned)c->num_cu * 4u;
    q.edge_row = grid;
  }
  const size_t rows = (size_t)grid + (sh ? edge_grid : 1u);
  const size_t need = rows * RD_SLOT + 128;                         // rows, then 64 doubles of bound constants, 64 of results
  {
    rc = regrow(c, &c->rd_slab, &c->rd_slab_cap, need, sizeof(double));
    if (rc) return rc;
  }
  if (rem) { rc = upload_rtab<T>(c, rem); if (rc) return rc; }   // (synchronous: the staging area is free again)
  RdParams<T> p;
  memset(&p, 0, sizeof(p));
  p.x = d_in; p.nfull = nfull; p.k = k;
  const double sf = scaling_factor(dtype, mx);
  p.sf = (T)sf;
  // the launch constants of k_compress (compress_pass): FastDiv where the host's windows allow it
  p.fast_sf = fast_sf_level(dtype, c->fastdiv, (double)p.sf, mn, mx, true);
  T* hb = reinterpret_cast<T*>(c->h_pin + PIN_TAB);
  for (int i = 0; i < k; i++) {                                   // (of fast_bw the window bit only: the probe keeps the range test)
    const FwdQuant<T> fq = fwd_quant<T>(ebs[i], c->fastdiv);
    hb[3 * i] = fq.range_min; hb[3 * i + 1] = fq.range_max; hb[3 * i + 2] = fq.bin_width;
    p.fast_bw |= (fq.fast_bw & 1u) << i;
  }
  double* d_bounds = c->rd_slab + rows * RD_SLOT;
  p.bounds = reinterpret_cast<const T*>(d_bounds);
  p.tab = tab_of<T>(c); p.rtab = reinterpret_cast<const T*>(c->rtab);
  p.slab = c->rd_slab;
  p.out = d_bounds + 64;
  HIPCHK(c, hipMemcpyAsync(d_bounds, hb, sizeof(T) * 3 * (size_t)k, hipMemcpyHostToDevice, s));
  if (sh) {
    q.rd = p;
    launch_ndrd_probe<T>(q, sh->nd == 2 ? GEOM_2D : GEOM_3D, (int)grid, (int)edge_grid, s);
  } else {
    launch_rd_probe<T>(p, (int)grid, rem, s);
  }
  HIPCHK(c, hipGetLastError());
  double* ho = reinterpret_cast<double*>(c->h_pin + PIN_TAB + 1024);
  HIPCHK(c, hipMemcpyAsync(ho, p.out, sizeof(double) * (2 + 2 * (size_t)k), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const double sf2 = (double)p.sf * (double)p.sf;
  const size_t nblk = sh ? sh->nblk : (n + 63) / 64;
  // the container's bytes before the entropy stage: bin ids (one per stream position), DC, AC_exact, header [, "DZND" trailer]
  const uint64_t fixed = (sh ? 64 * (uint64_t)nblk + 16 : (uint64_t)n) + 4 * (uint64_t)nblk + DCTZHIP_RD_HEADER_BYTES;
  for (int i = 0; i < k; i++) {
    uint64_t cnt;
    memcpy(&cnt, &ho[3 + 2 * i], sizeof(cnt));
    dctzhip_rd_point& r = pts[i];
    r.error_bound = ebs[i];
    r.cnt = cnt;
    r.sse = sf2 * ho[2 + 2 * i] / (double)c->rd_sse_div;
    r.psnr = psnr_of(ho[0], ho[1], r.sse, n);
    r.raw_bytes = fixed + 4 * cnt;
  }
  if (range) { range[0] = ho[0]; range[1] = ho[1]; }
  return DCTZHIP_OK;
}

static int rd_probe_checked(dctzhip_ctx* c, const void* d_in, size_t n, const NdShape* sh, int dtype, int k, const double* ebs,
                            dctzhip_rd_point* pts, double range[2]) {
  return dtype == DCTZHIP_F64 ? rd_probe_impl<double>(c, (const double*)d_in, n, sh, k, ebs, pts, range)
                              : rd_probe_impl<float>(c, (const float*)d_in, n, sh, k, ebs, pts, range);
}

// What dctzhip_rd_probe and dctzhip_rd_probe_nd ask of their arguments behind the shape
static int rd_probe_front(dctzhip_ctx* c, const char* what, const void* d_in, int k, const double* error_bounds, const dctzhip_rd_point* pts) {
  if (!d_in || !error_bounds || !pts) return fail(c, DCTZHIP_E_ARG, "%s: null pointer", what);
  if (!aligned16(d_in)) return fail(c, DCTZHIP_E_ARG, "%s: d_in must be 16-byte aligned", what);
  if (k < 1 || k > DCTZHIP_RD_MAXK) return fail(c, DCTZHIP_E_ARG, "%s: k = %d, must be 1 .. %d", what, k, DCTZHIP_RD_MAXK);
  for (int i = 0; i < k; i++)
    if (!(error_bounds[i] >= 1E-6)) return fail(c, DCTZHIP_E_BOUND, "ERROR BOUND is not acceptable");   // dctz-comp-lib.c:135-138
  return DCTZHIP_OK;
}

extern "C" int dctzhip_rd_probe(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, int k, const double* error_bounds,
                                dctzhip_rd_point* pts, double range[2]) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  rc = rd_probe_front(c, "dctzhip_rd_probe", d_in, k, error_bounds, pts);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return rd_probe_checked(c, d_in, n, nullptr, dtype, k, error_bounds, pts, range);
}

static size_t nd_elems(const NdShape& sh) { return sh.d[0] * sh.d[1] * sh.d[2]; }

extern "C" int dctzhip_rd_probe_nd(dctzhip_ctx* c, const void* d_in, int ndims, const size_t* dims, int dtype, int k,
                                   const double* error_bounds, dctzhip_rd_point* pts, double range[2]) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, DCTZHIP_EC, &sh);
  if (rc) return rc;
  rc = rd_probe_front(c, "dctzhip_rd_probe_nd", d_in, k, error_bounds, pts);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return rd_probe_checked(c, d_in, nd_elems(sh), &sh, dtype, k, error_bounds, pts, range);
}

// The candidate grid of dctzhip_compress_psnr, ascending: the doubles nearest to m * 10^e, e = -6 .. -1, then 1.
static constexpr int RD_GRID_N = 61;
static const char* const RD_MANT[10] = {"1", "1.25", "1.5", "2", "2.5", "3", "4", "5", "6", "8"};
static void rd_grid(double g[RD_GRID_N]) {
  int i = 0;
  for (int e = -6; e <= -1; e++)
    for (int m = 0; m < 10; m++) {
      char buf[32];
      snprintf(buf, sizeof(buf), "%se%d", RD_MANT[m], e);
      g[i++] = strtod(buf, nullptr);
    }
  g[i] = 1.0;
}

// The search of dctzhip_compress_psnr / dctzhip_compress_psnr_nd over the n elements of d_in.  The layout gives
//   probe(k, ebs, pts, range)   its rate-distortion probe,
//   compress(eb)                its ordinary compress into the caller's streams and *info,
//   decode(eb, d_rec)           its ordinary decode of those streams into d_rec (n elements).
template <typename Probe, typename Compress, typename Decode>
static int compress_psnr_search(dctzhip_ctx* c, const char* what, const void* d_in, size_t n, int dtype, double target_psnr,
                                double* error_bound_used, double* psnr_measured, Probe probe, Compress compress, Decode decode) {
  double g[RD_GRID_N];
  rd_grid(g);
  // call 1: the decade points 1e-6 .. 1 (grid indices 0, 10, ..., 60); the largest whose prediction reaches the target
  double ebs[DCTZHIP_RD_MAXK];
  dctzhip_rd_point pts[DCTZHIP_RD_MAXK];
  double range[2];
  for (int d = 0; d < 7; d++) ebs[d] = g[10 * d];
  int rc = probe(7, ebs, pts, range);
  if (rc) return rc;
  if (!std::isfinite(range[0]) || !std::isfinite(range[1]))
    return fail(c, DCTZHIP_E_ARG, "%s: the array's range is not finite (PSNR undefined)", what);
  if (range[0] == range[1]) return fail(c, DCTZHIP_E_ARG, "%s: constant array (PSNR undefined)", what);
  for (int d = 0; d < 7; d++)
    if (std::isnan(pts[d].sse)) return fail(c, DCTZHIP_E_ARG, "%s: the array holds a NaN (PSNR undefined)", what);
  int at = -1;
  for (int d = 6; d >= 0 && at < 0; d--)
    if (pts[d].psnr >= target_psnr) at = 10 * d;
  if (at < 0) return fail(c, DCTZHIP_E_BOUND, "%s: no error bound >= 1e-6 reaches %.3f dB", what, target_psnr);
  // call 2: the nine interior points above that decade point; the largest whose prediction reaches the target
  if (at < RD_GRID_N - 1) {
    for (int i = 0; i < 9; i++) ebs[i] = g[at + 1 + i];
    rc = probe(9, ebs, pts, nullptr);
    if (rc) return rc;
    for (int i = 8; i >= 0; i--)
      if (pts[i].psnr >= target_psnr) { at = at + 1 + i; break; }
  }
  // compress at the chosen point, decode into the context's scratch and measure; a miss steps down the grid
  const size_t es = elem_size(dtype);
  {
    char* r = (char*)c->rd_rec;
    rc = regrow(c, &r, &c->rd_rec_cap, n * es, 1);
    c->rd_rec = r;
    if (rc) return rc;
  }
  for (;; at--) {
    const double eb = g[at];
    rc = compress(eb);
    if (rc) return rc;
    rc = decode(eb, c->rd_rec);
    if (rc) return rc;
    double t[4];
    rc = dctzhip_psnr_terms(c, d_in, c->rd_rec, n, dtype, t);
    if (rc) return rc;
    const double psnr = psnr_of(t[0], t[1], t[3], n);
    *error_bound_used = eb;
    *psnr_measured = psnr;
    if (psnr >= target_psnr) return DCTZHIP_OK;
    if (at == 0) return fail(c, DCTZHIP_E_BOUND, "%s: measured %.3f dB at 1e-6, under the target %.3f dB", what, psnr, target_psnr);
    c->rd_stepdowns++;
  }
}

// What both target-PSNR calls ask of their pointers and the target
static int compress_psnr_front(dctzhip_ctx* c, const char* what, const void* d_in, const void* d_bin, const float* d_dc, const float* d_ac,
                               const dctzhip_cinfo* info, const double* error_bound_used, const double* psnr_measured, double target_psnr) {
  if (!d_in || !d_bin || !d_dc || !d_ac || !info || !error_bound_used || !psnr_measured) return fail(c, DCTZHIP_E_ARG, "%s: null pointer", what);
  if (!aligned16(d_in) || !aligned16(d_bin) || !aligned16(d_dc) || !aligned16(d_ac))
    return fail(c, DCTZHIP_E_ARG, "device buffers must be 16-byte aligned");
  if (!std::isfinite(target_psnr)) return fail(c, DCTZHIP_E_ARG, "%s: the target must be finite", what);
  return DCTZHIP_OK;
}

extern "C" int dctzhip_compress_psnr(dctzhip_ctx* c, const void* d_in, size_t n, int dtype, double target_psnr, void* d_bin,
                                     float* d_dc, float* d_ac, dctzhip_cinfo* info, double* error_bound_used, double* psnr_measured) {
  int rc = check_common(c, n, dtype, DCTZHIP_EC);
  if (rc) return rc;
  rc = compress_psnr_front(c, "dctzhip_compress_psnr", d_in, d_bin, d_dc, d_ac, info, error_bound_used, psnr_measured, target_psnr);
  if (rc) return rc;
  {
    Span sp[6];
    size_t m = 0;
    compress_spans(sp, &m, 0, d_in, n, dtype, d_bin, d_dc, d_ac, nullptr, nullptr);
    rc = check_spans(c, sp, m, "dctzhip_compress_psnr", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return compress_psnr_search(
      c, "dctzhip_compress_psnr", d_in, n, dtype, target_psnr, error_bound_used, psnr_measured,
      [&](int k, const double* ebs, dctzhip_rd_point* pts, double* range) { return rd_probe_checked(c, d_in, n, nullptr, dtype, k, ebs, pts, range); },
      [&](double eb) { return dctzhip_compress(c, d_in, n, dtype, eb, DCTZHIP_EC, d_bin, d_dc, d_ac, nullptr, nullptr, info); },
      [&](double eb, void* d_rec) { return dctzhip_decompress(c, d_bin, d_dc, d_ac, info->cnt, nullptr, n, dtype, eb, info->sf, DCTZHIP_EC, d_rec); });
}

extern "C" int dctzhip_compress_psnr_nd(dctzhip_ctx* c, const void* d_in, int ndims, const size_t* dims, int dtype, double target_psnr,
                                        void* d_bin, float* d_dc, float* d_ac, dctzhip_cinfo* info, double* error_bound_used,
                                        double* psnr_measured) {
  NdShape sh;
  int rc = nd_front(c, ndims, dims, dtype, DCTZHIP_EC, &sh);
  if (rc) return rc;
  rc = compress_psnr_front(c, "dctzhip_compress_psnr_nd", d_in, d_bin, d_dc, d_ac, info, error_bound_used, psnr_measured, target_psnr);
  if (rc) return rc;
  const size_t n = nd_elems(sh);
  {
    Span sp[4];                                        // the array, and the streams' 64 nblk positions as dctzhip_compress_nd writes them
    size_t m = 0;
    add_span(sp, &m, d_in, n * elem_size(dtype), SPAN_READ, 0);
    add_span(sp, &m, d_bin, sh.nblk * 64, SPAN_OUT, 0);
    add_span(sp, &m, d_dc, sh.nblk * sizeof(float), SPAN_OUT, 0);
    add_span(sp, &m, d_ac, sh.nblk * 64 * sizeof(float), SPAN_OUT, 0);
    rc = check_spans(c, sp, m, "dctzhip_compress_psnr_nd", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return compress_psnr_search(
      c, "dctzhip_compress_psnr_nd", d_in, n, dtype, target_psnr, error_bound_used, psnr_measured,
      [&](int k, const double* ebs, dctzhip_rd_point* pts, double* range) { return rd_probe_checked(c, d_in, n, &sh, dtype, k, ebs, pts, range); },
      [&](double eb) { return dctzhip_compress_nd(c, d_in, ndims, dims, dtype, eb, DCTZHIP_EC, d_bin, d_dc, d_ac, nullptr, info); },
      [&](double eb, void* d_rec) {
        return dctzhip_decompress_nd(c, d_bin, d_dc, d_ac, info->cnt, nullptr, ndims, dims, dtype, eb, info->sf, DCTZHIP_EC, d_rec);
      });
}

// ---- batches of arrays (include/dctz_hip.h: dctzhip_compress_batch / dctzhip_decompress_batch) ---------------------
// The reference's own workloads are lists of small arrays, one dctz_compress call each (tests/test-dctz.sh:13-56 over
// tests/list-msst19.txt:1-6: 12 960 ... 37 024 doubles).  One such call is four or five launches and a host hand-off
// around a few microseconds of kernel work; a batch puts the arrays of one element type through ONE launch sequence
// (statistics -> scaling factors -> block DCT + binning -> remainder blocks -> [QT maxima] -> list placement -> scaled
// copies) with ONE hand-off, every workgroup running the single-array body on its array's own parameter block.
static constexpr int BATCH_MAX = 1024;                    // arrays per launch sequence (longer batches: several sequences, one hand-off)
static constexpr size_t BATCH_BIG = (size_t)1 << 24;      // arrays from this size on take the single-array path (fused statistics)

template <typename T>
static int rtab_for(dctzhip_ctx* c, int l, const T** out) {
  const int dt = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  if (!c->rtab_cache[dt][l]) {
    T h[RTAB_SIZE];
    fill_rem_tab<T>(l, h);
    void* d = nullptr;
    HIPCHK(c, hipMalloc(&d, sizeof(T) * RTAB_SIZE));
    HIPCHK(c, hipMemcpy(d, h, sizeof(T) * RTAB_SIZE, hipMemcpyHostToDevice));
    c->rtab_cache[dt][l] = d;
  }
  *out = reinterpret_cast<const T*>(c->rtab_cache[dt][l]);
  return DCTZHIP_OK;
}

static int ensure_batch(dctzhip_ctx* c, size_t K, size_t blob_bytes, size_t res_bytes) {
  if (K > c->b_cap) {
    const size_t cap = K + K / 2 + 16;
    void* old[] = {c->b_ctl, c->b_guess, c->b_stats, c->b_remcnt};
    for (void* b : old) if (b) HIPCHK(c, hipFree(b));
    c->b_ctl = nullptr; c->b_guess = nullptr; c->b_stats = nullptr; c->b_remcnt = nullptr; c->b_cap = 0;
    HIPCHK(c, hipMalloc(&c->b_ctl, cap * sizeof(Ctl)));
    HIPCHK(c, hipMalloc(&c->b_guess, cap * sizeof(SfGuess)));
    HIPCHK(c, hipMalloc(&c->b_stats, cap * 3 * sizeof(double)));
    HIPCHK(c, hipMalloc(&c->b_remcnt, cap * sizeof(unsigned)));
    c->b_cap = cap;
    c->b_ctl_dirty = 1;
  }
  if (blob_bytes > c->b_blob_cap) {
    const size_t cap = (blob_bytes + blob_bytes / 2 + 4095) & ~(size_t)4095;
    if (c->b_blob) HIPCHK(c, hipHostFree(c->b_blob));
    if (c->b_blob_dev) HIPCHK(c, hipFree(c->b_blob_dev));
    c->b_blob = nullptr; c->b_blob_dev = nullptr; c->b_blob_cap = 0;
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->b_blob), cap, hipHostMallocCoherent | hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->b_blob_hdev), c->b_blob, 0));
    HIPCHK(c, hipMalloc(&c->b_blob_dev, cap));
    c->b_blob_cap = cap;
  }
  if (res_bytes > c->b_res_cap) {
    const size_t cap = (res_bytes + res_bytes / 2 + 4095) & ~(size_t)4095;
    if (c->b_res) HIPCHK(c, hipHostFree(c->b_res));
    c->b_res = nullptr; c->b_res_cap = 0;
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->b_res), cap, hipHostMallocCoherent | hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->b_res_hdev), c->b_res, 0));
    c->b_res_cap = cap;
  }
  return DCTZHIP_OK;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// share of `cap` workgroups an array of `ntiles` tiles gets when the whole sequence has `total` tiles (>= 1 per array
// that has a tile; never more than its tiles)
static unsigned share_of(unsigned ntiles, size_t total, unsigned cap) {
  if (ntiles == 0) return 0;
  if (total <= cap) return ntiles;
  const unsigned g = (unsigned)((size_t)cap * ntiles / total);
  return g < 1 ? 1u : (g > ntiles ? ntiles : g);
}

namespace {
struct SeqC {                       // one launch sequence of a compress batch: arrays idx[] (all of one element type)
  std::vector<int> idx;
  int dtype = 0;
  std::vector<unsigned> nfull, rem, ntiles, G, nparts, part_base, tile_base, list_base, scale_wgs, stats_wgs, sample, main_part_base;
  size_t parts_all = 0;            // statistics partials + (fused) the main kernels' partials
  bool fused = false;              // the sequence has speculative items: k_compress_batch<STATS>, true statistics into main_part_base
  size_t tiles_total = 0, lists_total = 0, parts_total = 0;
  unsigned grid_main = 0, grid_list = 0, grid_scale = 0, grid_stats = 0, nrem = 0;
  size_t blob_off = 0, blob_bytes = 0, item_off = 0;    // item_off: first array of this sequence in b_ctl / b_guess / b_stats / results
  int chain = 0;
};
// A mixed batch runs as two CHAINS of sequences side by side -- fp64 on the context's stream, fp32 on a second one --
// each with its own region of the scratch buffers and its own mailbox word; sequences of one chain follow each other
// and reuse the chain's region.
struct Chain {
  hipStream_t s = nullptr;
  size_t tile_off = 0, list_off = 0, part_off = 0;                    // first tile slot / list-length entry / partial slot
  volatile unsigned long long* word = nullptr;                         // host view of the mailbox word the chain's last sequence publishes
  volatile unsigned long long* word_dev = nullptr;
  int last = -1;                                                       // index of the chain's last sequence
};
struct SeqD {
  std::vector<int> idx;
  int dtype = 0;
  std::vector<unsigned> nfull, rem, ntiles, nwg, tile_base, wg_base;
  size_t tiles_total = 0, wgs_total = 0;
  unsigned grid_cnt = 0, grid_main = 0, nrem = 0;
  size_t blob_off = 0, blob_bytes = 0, item_off = 0;
  int chain = 0;
};
}  // namespace

// fork: the second chain's stream starts behind everything queued on the context's stream so far
static int chains_fork(dctzhip_ctx* c, Chain* ch, bool two) {
  ch[0].s = c->stream; ch[1].s = c->stream;
  ch[0].word = &c->box->seq_done; ch[0].word_dev = &c->box_dev->seq_done;
  ch[1].word = &c->box->seq_stats; ch[1].word_dev = &c->box_dev->seq_stats;
  if (!two) return DCTZHIP_OK;
  if (!c->b_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->b_stream, hipStreamNonBlocking));
  if (!c->b_fork) HIPCHK(c, hipEventCreateWithFlags(&c->b_fork, hipEventDisableTiming));
  if (!c->b_join) HIPCHK(c, hipEventCreateWithFlags(&c->b_join, hipEventDisableTiming));
  ch[1].s = c->b_stream;
  HIPCHK(c, hipEventRecord(c->b_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->b_stream, c->b_fork, 0));
  return DCTZHIP_OK;
}
// join: whatever is queued on the context's stream after the call runs behind both chains
static int chains_join(dctzhip_ctx* c, bool two) {
  if (!two) return DCTZHIP_OK;
  HIPCHK(c, hipEventRecord(c->b_join, c->b_stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->b_join, 0));
  return DCTZHIP_OK;
}

template <typename T>
static void plan_compress(dctzhip_ctx* c, const dctzhip_batch_citem* items, int mode, SeqC& q, unsigned cap_div) {
  const size_t k = q.idx.size();
  constexpr int EPV = Traits<T>::EPV;
  unsigned cap = (unsigned)(c->num_cu * wg_per_cu<T>(c, false, mode, false, GEOM_1D)) / cap_div;      // (two chains share the chip)
  if (c->grid_c > 0 && (unsigned)c->grid_c < cap) cap = (unsigned)c->grid_c;
  cap = cap > 2 * (unsigned)k ? cap - (unsigned)k : cap / 2 + 1;      // (every array with a tile gets at least one workgroup)
  size_t tiles = 0;
  q.nfull.resize(k); q.rem.resize(k); q.ntiles.resize(k); q.G.resize(k); q.nparts.resize(k); q.part_base.resize(k);
  q.tile_base.resize(k); q.list_base.resize(k); q.scale_wgs.resize(k); q.stats_wgs.resize(k); q.sample.assign(k, 0u); q.main_part_base.assign(k, 0u);
  for (size_t j = 0; j < k; j++) {
    const size_t n = items[q.idx[j]].n;
    q.nfull[j] = (unsigned)(n / 64); q.rem[j] = (unsigned)(n % 64);
    q.ntiles[j] = (q.nfull[j] + TILE_BLKS - 1) / TILE_BLKS;
    tiles += q.ntiles[j];
  }
  const unsigned maxp = (unsigned)((size_t)(PART_SLOTS - 64) / k) < 1u ? 1u : (unsigned)((size_t)(PART_SLOTS - 64) / k);
  for (size_t j = 0; j < k; j++) {
    const size_t n = items[q.idx[j]].n;
    q.G[j] = share_of(q.ntiles[j], tiles, cap);
    const size_t nvec = n / EPV;
    size_t sg = (nvec + SWG * 4 - 1) / (SWG * 4);          // the single-array path's statistics grid (same partials, same sum)
    if (sg < 1) sg = 1;
    if (sg > (size_t)c->stats_grid) sg = (size_t)c->stats_grid;
    if (sg > maxp) sg = maxp;
    // The same input under several error bounds (what the reference's own driver does: tests/test-dctz.sh:13-56 loops the
    // bounds over each file): calc_data_stat (util.c:12-44) does not depend on the bound, so the statistics pass reads the
    // array once -- the later items of the sequence take the first one's partials (every item still gets its own choice of
    // sf and its own record).  In-place scaling (k_scale_batch) runs behind everything else of the sequence.
    size_t own = j;
    for (size_t i = 0; i < j && k <= 256; i++)
      if (items[q.idx[i]].d_in == items[q.idx[j]].d_in && items[q.idx[i]].n == n) { own = i; break; }
    // Speculation, as on the single-array path: an item from spec_min elements on gets its scaling
    // factor from a sample (one chunk of 4 KiB out of every spec_group), k_compress_batch<STATS> takes the true statistics
    // while it streams the array, and the host's check of the device's choice below -- it has been there for every item since
    // round 3 -- is then the check of the guess: an item it refuses is done again on its own.  Not for an item that is scaled
    // in place (k_scale_batch would have divided the input by the wrong factor by then).
    constexpr size_t chunk = (size_t)SWG * EPV;
    const bool in_place = items[q.idx[j]].d_scaled && items[q.idx[j]].d_scaled == items[q.idx[j]].d_in;
    if (c->speculate && c->batch_speculate && c->b_spec_now && !in_place && q.ntiles[j] && n >= c->spec_min && n >= 4 * chunk * c->spec_group) {
      q.sample[j] = (unsigned)c->spec_group;
      const size_t ngroups = n / chunk / c->spec_group;
      const size_t scap = (size_t)(c->stats_grid > 1 ? c->stats_grid / 2 : 1);
      sg = ngroups < scap ? ngroups : scap;
      if (sg > maxp) sg = maxp;
      if (sg < 1) sg = 1;
    }
    if (own != j && q.sample[own] == q.sample[j]) { q.nparts[j] = q.nparts[own]; q.part_base[j] = q.part_base[own]; q.stats_wgs[j] = 0; }
    else { q.nparts[j] = (unsigned)sg; q.part_base[j] = (unsigned)q.parts_total; q.parts_total += sg; q.stats_wgs[j] = (unsigned)sg; }
    if (q.sample[j]) q.fused = true;
    q.tile_base[j] = (unsigned)q.tiles_total; q.tiles_total += q.ntiles[j] + 1;     // + the remainder block's list
    q.list_base[j] = (unsigned)q.lists_total; q.lists_total += q.G[j] + 1;
    q.grid_main += q.G[j];
    q.grid_list += q.G[j] + (q.rem[j] ? 1u : 0u);
    q.nrem += q.rem[j] ? 1u : 0u;
    unsigned sw = 0;
    if (items[q.idx[j]].d_scaled) { size_t w = (nvec + SWG * 4 - 1) / (SWG * 4); sw = (unsigned)(w < 1 ? 1 : (w > 256 ? 256 : w)); }
    q.scale_wgs[j] = sw; q.grid_scale += sw;
  }
  q.grid_stats = (unsigned)q.parts_total;
  if (q.fused) {
    size_t at = q.parts_total;
    for (size_t j = 0; j < k; j++) { q.main_part_base[j] = (unsigned)at; at += q.G[j] + 1; }
    if (at > (size_t)PART_SLOTS) {                    // no room for the main kernels' partials: the sequence takes the full passes
      q.fused = false;
      q.parts_total = 0; q.grid_stats = 0;
      std::fill(q.sample.begin(), q.sample.end(), 0u);
      for (size_t j = 0; j < k; j++) {                // (as above, without the speculation)
        const size_t n = items[q.idx[j]].n;
        size_t sg = (n / EPV + SWG * 4 - 1) / (SWG * 4);
        if (sg < 1) sg = 1;
        if (sg > (size_t)c->stats_grid) sg = (size_t)c->stats_grid;
        if (sg > maxp) sg = maxp;
        size_t own = j;
        for (size_t i = 0; i < j && k <= 256; i++)
          if (items[q.idx[i]].d_in == items[q.idx[j]].d_in && items[q.idx[i]].n == n) { own = i; break; }
        if (own != j) { q.nparts[j] = q.nparts[own]; q.part_base[j] = q.part_base[own]; q.stats_wgs[j] = 0; }
        else { q.nparts[j] = (unsigned)sg; q.part_base[j] = (unsigned)q.parts_total; q.parts_total += sg; q.stats_wgs[j] = (unsigned)sg; }
      }
      q.grid_stats = (unsigned)q.parts_total;
    } else {
      q.parts_all = at;
    }
  }
  q.blob_bytes = align16(k * sizeof(BatchFwd<T>)) + align16(4 * (k + 1) * sizeof(unsigned) + (size_t)q.nrem * sizeof(unsigned));
}

template <typename T>
static int launch_compress_seq(dctzhip_ctx* c, const dctzhip_batch_citem* items, int mode, const SeqC& q, const Chain& ch, bool publish,
                               unsigned long long seq, bool first_of_dtype) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  const size_t k = q.idx.size();
  hipStream_t s = ch.s;
  // launch-time checks of the plan against the buffers it indexes
  if (q.parts_total > (size_t)PART_SLOTS || q.parts_all > (size_t)PART_SLOTS || ch.list_off + q.lists_total + 2 > c->tile_cap || ch.tile_off + q.tiles_total > c->qcnt_cap)
    return fail(c, DCTZHIP_E_INTERNAL, "batch: scratch plan exceeds its buffers");
  unsigned char* hb = c->b_blob + q.blob_off;
  BatchFwd<T>* hi = reinterpret_cast<BatchFwd<T>*>(hb);
  unsigned* hfirst = reinterpret_cast<unsigned*>(hb + align16(k * sizeof(BatchFwd<T>)));
  unsigned* f_stats = hfirst, *f_main = hfirst + (k + 1), *f_list = hfirst + 2 * (k + 1), *f_scale = hfirst + 3 * (k + 1);
  unsigned* rem_items = hfirst + 4 * (k + 1);
  const size_t first_off = align16(k * sizeof(BatchFwd<T>));
  unsigned a_stats = 0, a_main = 0, a_list = 0, a_scale = 0, nrem = 0;
  for (size_t j = 0; j < k; j++) {
    const dctzhip_batch_citem& it = items[q.idx[j]];
    const double eb = it.error_bound;
    BatchFwd<T>& b = hi[j];
    memset(&b, 0, sizeof(b));
    FwdParams<T>& p = b.p;
    p.x = (const T*)it.d_in; p.bin = (uint8_t*)it.d_bin_index; p.dc = it.d_dc; p.ac = it.d_ac_exact; p.coef = nullptr; p.scaled = nullptr;
    const size_t slot0 = (ch.tile_off + (size_t)q.tile_base[j]) * TILE_ELEMS;
    p.ac_tmp = c->ac_tmp ? c->ac_tmp + slot0 : nullptr;
    // (the chain's region starts at a byte offset that is right for either element type)
    p.qt_item = c->qt_item ? reinterpret_cast<T*>((char*)c->qt_item + ch.tile_off * TILE_ELEMS * sizeof(double)) + (size_t)q.tile_base[j] * TILE_ELEMS : nullptr;
    p.qt_j = c->qt_j ? c->qt_j + slot0 : nullptr;
    p.tile_cnt = c->tile_cnt + ch.list_off + q.list_base[j];
    p.qcnt = c->qcnt + (ch.tile_off + (size_t)q.tile_base[j]) * TILE_BLKS; p.ttot = c->ttot + ch.tile_off + q.tile_base[j];
    p.tab = tab_of<T>(c); p.rtab = nullptr;
    if (q.rem[j]) { int rc = rtab_for<T>(c, (int)q.rem[j], &p.rtab); if (rc) return rc; }
    p.ctl = c->b_ctl + q.item_off + j;
    p.guess = c->b_guess + q.item_off + j;           // the scaling factor is chosen on the device (k_sf_batch), verified afterwards
    p.stat_part = q.fused ? c->part + 3 * (ch.part_off + (size_t)q.main_part_base[j]) : nullptr;
    p.nfull = q.nfull[j]; p.ntiles = q.ntiles[j]; p.last_is_full = q.rem[j] ? 0u : 1u;
    p.nlists_main = q.G[j];
    p.sf = (T)1; p.fast_sf = 0;                       // (placeholders: p.guess is set)
    set_quant(p, fwd_quant<T>(eb, c->fastdiv));
    b.eb = eb; b.scaled = (T*)it.d_scaled; b.n = (unsigned)it.n; b.rem = q.rem[j];
    b.nlists = q.G[j] + (q.rem[j] ? 1u : 0u);
    b.nparts = q.nparts[j]; b.part_base = q.part_base[j]; b.sample = q.sample[j];
    f_stats[j] = a_stats; a_stats += q.stats_wgs[j];
    f_main[j] = a_main; a_main += q.G[j];
    f_list[j] = a_list; a_list += b.nlists;
    f_scale[j] = a_scale; a_scale += q.scale_wgs[j];
    if (q.rem[j]) rem_items[nrem++] = (unsigned)j;
  }
  f_stats[k] = a_stats; f_main[k] = a_main; f_list[k] = a_list; f_scale[k] = a_scale;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);             // the table is complete in host memory before the first launch reads it

  const BatchFwd<T>* it_h = reinterpret_cast<const BatchFwd<T>*>(c->b_blob_hdev + q.blob_off);
  const unsigned* first_h = reinterpret_cast<const unsigned*>(c->b_blob_hdev + q.blob_off + first_off);
  unsigned char* db = c->b_blob_dev + q.blob_off;
  const BatchFwd<T>* it_d = reinterpret_cast<const BatchFwd<T>*>(db);
  const unsigned* first_d = reinterpret_cast<const unsigned*>(db + first_off);
  const bool prof = c->profiling && first_of_dtype;
  hipEvent_t* ev = c->b_ev[dtype];
  if (prof) for (int i = 0; i < 5; i++) if (!ev[i]) HIPCHK(c, hipEventCreate(&ev[i]));
  if (prof) HIPCHK(c, hipEventRecord(ev[0], s));
  double* part = c->part + 3 * ch.part_off;
  launch_stats_batch<T>(it_h, first_h, (unsigned)k, q.grid_stats, c->b_blob_hdev + q.blob_off, db, q.blob_bytes, part, s);
  const SfTable tab = {c->sf_thr[dtype], c->sf_pw[dtype], c->sf_nk[dtype], c->fastdiv, dtype};
  launch_sf_batch<T>(it_d, (unsigned)k, part, c->b_stats + 3 * q.item_off, tab, s);
  if (prof) HIPCHK(c, hipEventRecord(ev[1], s));
  if (q.grid_main) {
    launch_compress_batch<T>(it_d, first_d + (k + 1), (unsigned)k, q.grid_main, mode, q.fused, s);
    SET_LAST(c, sizeof(T) == 8 ? 2 : 3, "k_compress_batch<%s, %d, %s>", tname<T>(), mode, q.fused ? "true" : "false");
  }
  if (prof) HIPCHK(c, hipEventRecord(ev[2], s));
  if (nrem) launch_compress_rem_batch<T>(it_d, first_d + 4 * (k + 1), nrem, mode, s);
  BatchFin fin;
  fin.word = publish ? const_cast<unsigned long long*>(ch.word_dev) : nullptr; fin.seq = seq;
  fin.res = c->b_res_hdev + q.item_off * sizeof(BatchResC);
  fin.resq = mode == DCTZHIP_QT ? reinterpret_cast<BatchResQ*>(c->b_res_hdev + c->b_cap * sizeof(BatchResC)) + q.item_off : nullptr;
  // (every array has at least one list or a remainder block: n >= 1)
  unsigned chunks = 1;                               // second grid dimension: chunks of tiles of the longest list (one tile per wave)
  for (size_t j = 0; j < k; j++)
    if (q.G[j]) { const unsigned per = (q.ntiles[j] + q.G[j] - 1) / q.G[j], ch = (per + SWG / 64 - 1) / (SWG / 64); if (ch > chunks) chunks = ch; }
  launch_compact_batch<T>(it_d, first_d + 2 * (k + 1), (unsigned)k, q.grid_list, chunks, mode, c->b_stats + 3 * q.item_off, fin, s);
  if (prof) HIPCHK(c, hipEventRecord(ev[3], s));
  if (q.grid_scale) launch_scale_batch<T>(it_d, first_d + 3 * (k + 1), (unsigned)k, q.grid_scale, s);
  if (prof) HIPCHK(c, hipEventRecord(ev[4], s));
  HIPCHK(c, hipGetLastError());
  return DCTZHIP_OK;
}

static int batch_timings(dctzhip_ctx* c, int dtype) {
  hipEvent_t* ev = c->b_ev[dtype];
  HIPCHK(c, hipEventSynchronize(ev[4]));
  float a = 0, b = 0, d = 0, e = 0;
  HIPCHK(c, hipEventElapsedTime(&a, ev[0], ev[1]));
  HIPCHK(c, hipEventElapsedTime(&b, ev[1], ev[2]));
  HIPCHK(c, hipEventElapsedTime(&d, ev[2], ev[3]));
  HIPCHK(c, hipEventElapsedTime(&e, ev[3], ev[4]));
  c->b_last[dtype].stats_ms = a; c->b_last[dtype].main_ms = b; c->b_last[dtype].tail_ms = d + e; c->b_last[dtype].total_ms = a + b + d + e;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_last_batch_timings(dctzhip_ctx* c, dctzhip_timings t[2]) {
  if (!c || !t) return DCTZHIP_E_ARG;
  if (!c->b_have_timings) return fail(c, DCTZHIP_E_ARG, "no batch timings recorded (enable profiling first)");
  t[0] = c->b_last[0]; t[1] = c->b_last[1];
  return DCTZHIP_OK;
}

// ---- batches through the one-launch kernels ---------------------------------------------------------------------------
// The arrays of one element type whose workgroups all fit the chip at once -- ONE_TW tiles per workgroup, as in
// compress_one -- share ONE launch: every array has its own workgroups, its own stretch of the board and its own entry of
// the result table, and the host waits for every entry's tag.  A mixed batch is two launches one after the other on the
// context's stream (two kernels that both need all their workgroups resident must not share the chip).  Arrays that do
// not fit, and every array when such a launch gives up, go through the chain of batch kernels below, as before.
static int wait_tags(dctzhip_ctx* c, const volatile unsigned* first, size_t stride_bytes, size_t k, unsigned tag, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  size_t at = 0;
  for (unsigned long long spins = 1; at < k; spins++) {
    const volatile unsigned* w = reinterpret_cast<const volatile unsigned*>(reinterpret_cast<const volatile char*>(first) + at * stride_bytes);
    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == tag) { at++; continue; }
    __builtin_ia32_pause();
    if ((spins & 0xFFFF) == 0) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == tag) continue;
        return fail(c, DCTZHIP_E_INTERNAL, "%s: stream drained without publishing its results", what);
      }
      if (q != hipErrorNotReady) return fail(c, DCTZHIP_E_HIP, "%s: %s", what, hipGetErrorString(q));
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) return fail(c, DCTZHIP_E_INTERNAL, "%s: no result after 10 s", what);
    }
  }
  return DCTZHIP_OK;
}
namespace {
struct OnePlan { std::vector<int> idx; std::vector<unsigned> nwg; unsigned grid = 0; bool scaled = false; size_t item_off = 0, rec_off = 0; };
}
static unsigned one_wgs_of(size_t n) {
  const unsigned nfull = (unsigned)(n / 64), ntiles = (nfull + TILE_BLKS - 1) / TILE_BLKS;
  return (ntiles + ONE_TW - 1) / ONE_TW + ((n % 64) ? 1u : 0u);
}
static int ensure_one_bctl(dctzhip_ctx* c, size_t K) {
  if (K <= c->one_bctl_cap) return DCTZHIP_OK;
  const size_t cap = K + K / 2 + 16;
  if (c->one_bctl) HIPCHK(c, hipFree(c->one_bctl));
  c->one_bctl = nullptr; c->one_bctl_cap = 0;
  HIPCHK(c, hipMalloc(&c->one_bctl, 2 * cap * sizeof(Ctl)));
  HIPCHK(c, hipMemset(c->one_bctl, 0, 2 * cap * sizeof(Ctl)));
  if (c->one_bqt) HIPCHK(c, hipFree(c->one_bqt));
  c->one_bqt = nullptr;
  HIPCHK(c, hipMalloc(&c->one_bqt, 2 * cap * 64 * sizeof(unsigned long long)));
  HIPCHK(c, hipMemset(c->one_bqt, 0, 2 * cap * 64 * sizeof(unsigned long long)));
  c->one_bctl_cap = cap; c->one_bdirty[0] = c->one_bdirty[1] = 0;
  return DCTZHIP_OK;
}

template <typename T>
static int fill_one_recs_c(dctzhip_ctx* c, const dctzhip_batch_citem* items, const OnePlan& pl, OneRecC* recs) {
  unsigned base = 0;
  size_t at = 0;
  for (size_t j = 0; j < pl.idx.size(); j++) {
    const dctzhip_batch_citem& it = items[pl.idx[j]];
    const double eb = it.error_bound;
    OneRecC r;
    memset(&r, 0, sizeof(r));
    r.x = it.d_in; r.bin = it.d_bin_index; r.dc = it.d_dc; r.ac = it.d_ac_exact; r.scaled = it.d_scaled;
    r.nfull = (unsigned)(it.n / 64); r.rem = (unsigned)(it.n % 64); r.ntiles = (r.nfull + TILE_BLKS - 1) / TILE_BLKS;
    if (r.rem) { const T* rt = nullptr; int rc = rtab_for<T>(c, (int)r.rem, &rt); if (rc) return rc; r.rtab = rt; }
    set_quant(r, fwd_quant<T>(eb, c->fastdiv));
    r.eb = eb;
    r.nwg = pl.nwg[j]; r.board_base = base; r.item = (unsigned)(pl.item_off + j);
    for (unsigned w = 0; w < pl.nwg[j]; w++) { r.wg_local = w; recs[at++] = r; }
    base += pl.nwg[j];
  }
  return DCTZHIP_OK;
}

static int batch_one_compress(dctzhip_ctx* c, int k, const dctzhip_batch_citem* items, int mode, dctzhip_cinfo* infos, std::vector<char>& done) {
  c->b_one_seen[0] = c->b_one_seen[1] = 0;
  if (!c->one || !c->handoff || !c->dev_sf) return DCTZHIP_OK;
  if (c->one_cooldown > 0) { c->one_cooldown--; return DCTZHIP_OK; }
  OnePlan pl[2];
  size_t K = 0, nrec = 0;
  for (int dt = 1; dt >= 0; dt--) {
    OnePlan& q = pl[dt];
    if (c->sf_nk[dt] <= 0 || c->sf_nk[dt] > 64 * (dt == DCTZHIP_F64 ? 10 : 2)) continue;
    for (int i = 0; i < k; i++) {
      if (items[i].dtype != dt || items[i].n >= BATCH_BIG) continue;
      // (an array whose scaled copy goes over its input takes the chain: compress_one says why)
      if (items[i].d_scaled && items[i].d_scaled == items[i].d_in) continue;
      q.idx.push_back(i); q.nwg.push_back(one_wgs_of(items[i].n)); q.grid += q.nwg.back();
      q.scaled = q.scaled || items[i].d_scaled != nullptr;
    }
    const unsigned cap = dt == DCTZHIP_F64 ? one_capacity<double>(c, false, mode, q.scaled) : one_capacity<float>(c, false, mode, q.scaled);
    if (q.idx.empty() || q.grid > cap || q.grid > (unsigned)ONE_BOARD) { q.idx.clear(); q.nwg.clear(); q.grid = 0; continue; }
    q.item_off = K; K += q.idx.size();
    q.rec_off = nrec; nrec += q.grid;
  }
  if (K == 0) return DCTZHIP_OK;
  int rc = ensure_batch(c, K, nrec * sizeof(OneRecC), 0);
  if (rc) return rc;
  rc = ensure_batch(c, K, nrec * sizeof(OneRecC), c->b_cap * (sizeof(BatchResC) + (mode == DCTZHIP_QT ? sizeof(BatchResQ) : 0)));
  if (rc) return rc;
  rc = ensure_one_bctl(c, K);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const unsigned h = c->one_bslot;
  if (mode == DCTZHIP_QT) c->one_bslot ^= 1u;
  if (c->one_bdirty[h] > 0) {                        // (entries a call with more arrays than its successor left behind)
    HIPCHK(c, hipMemsetAsync(c->one_bqt + (size_t)h * c->one_bctl_cap * 64, 0, c->one_bctl_cap * 64 * sizeof(unsigned long long), s));
    c->one_bdirty[h] = 0;
  }
  const unsigned tag = (unsigned)(++c->seq) | 0x80000000u;
  BatchResC* res = reinterpret_cast<BatchResC*>(c->b_res);
  BatchResQ* resq_h = reinterpret_cast<BatchResQ*>(c->b_res + c->b_cap * sizeof(BatchResC));
  for (size_t i = 0; i < K; i++) res[i].pad = 0;
  OneRecC* recs = reinterpret_cast<OneRecC*>(c->b_blob);
  for (int dt = 1; dt >= 0; dt--) {
    if (pl[dt].idx.empty()) continue;
    rc = dt == DCTZHIP_F64 ? fill_one_recs_c<double>(c, items, pl[dt], recs + pl[dt].rec_off) : fill_one_recs_c<float>(c, items, pl[dt], recs + pl[dt].rec_off);
    if (rc) return rc;
  }
  __atomic_thread_fence(__ATOMIC_SEQ_CST);             // records and cleared tags are in host memory before the launches read them
  for (int dt = 1; dt >= 0; dt--) {
    const OnePlan& q = pl[dt];
    if (q.idx.empty()) continue;
    const unsigned epoch = one_next_epoch(c);
    if (!epoch) { (void)one_gave_up(c); c->one_bdirty[0] = c->one_bdirty[1] = (unsigned)c->one_bctl_cap; return DCTZHIP_E_HIP; }
    const bool prof = c->profiling != 0;
    hipEvent_t* ev = c->b_ev[dt];
    if (prof) { for (int i = 0; i < 5; i++) if (!ev[i]) HIPCHK(c, hipEventCreate(&ev[i])); HIPCHK(c, hipEventRecord(ev[0], s)); HIPCHK(c, hipEventRecord(ev[1], s)); }
    OneBoard b;
    b.ga = c->one_ga; b.gb = c->one_gb; b.rec = c->one_rec; b.epoch = epoch; b.nwg = 0; b.dbg = nullptr;
    const SfTable sft = {c->sf_thr[dt], c->sf_pw[dt], c->sf_nk[dt], c->fastdiv, dt};
    BatchResC* res_d = reinterpret_cast<BatchResC*>(c->b_res_hdev);
    BatchResQ* resq_d = mode == DCTZHIP_QT ? reinterpret_cast<BatchResQ*>(c->b_res_hdev + c->b_cap * sizeof(BatchResC)) : nullptr;
    const OneRecC* recs_d = reinterpret_cast<const OneRecC*>(c->b_blob_hdev) + q.rec_off;
    Ctl* ctl = c->one_bctl;
    unsigned long long* qt = c->one_bqt + (size_t)h * c->one_bctl_cap * 64;
    unsigned long long* qt_next = c->one_bqt + (size_t)(h ^ 1u) * c->one_bctl_cap * 64;
    if (dt == DCTZHIP_F64) {
      OneBatchC<double> cm = {recs_d, c->tab_f64, ctl, qt, qt_next, b, sft, res_d, resq_d, tag, (unsigned)c->one_bad_guess | (c->one_withhold ? 16u : 0u)};
      launch_compress_one_batch<double>(cm, q.grid, mode, q.scaled, s);
      SET_LAST(c, 2, "k_compress_one_batch<double, %d, %s>", mode, bname(q.scaled));
    } else {
      OneBatchC<float> cm = {recs_d, c->tab_f32, ctl, qt, qt_next, b, sft, res_d, resq_d, tag, (unsigned)c->one_bad_guess | (c->one_withhold ? 16u : 0u)};
      launch_compress_one_batch<float>(cm, q.grid, mode, q.scaled, s);
      SET_LAST(c, 3, "k_compress_one_batch<float, %d, %s>", mode, bname(q.scaled));
    }
    if (prof) { HIPCHK(c, hipEventRecord(ev[2], s)); HIPCHK(c, hipEventRecord(ev[3], s)); HIPCHK(c, hipEventRecord(ev[4], s)); }
    HIPCHK(c, hipGetLastError());
    c->one_calls++;
    c->b_one_seen[dt] = 1;
  }
  // this call's half: dirty where QT maxima were merged (EC leaves it clean); the other half: its first K entries are zeroed
  if (mode == DCTZHIP_QT) c->one_bdirty[h] = (unsigned)K;
  if (mode == DCTZHIP_QT && c->one_bdirty[h ^ 1u] <= K) c->one_bdirty[h ^ 1u] = 0;
  rc = wait_tags(c, &res[0].pad, sizeof(BatchResC), K, tag, "compress batch (one launch)");
  if (rc) { (void)one_gave_up(c); c->one_bdirty[0] = c->one_bdirty[1] = (unsigned)c->one_bctl_cap; return rc; }
  if (c->profiling) {
    c->b_last[0] = dctzhip_timings{0, 0, 0, 0}; c->b_last[1] = dctzhip_timings{0, 0, 0, 0};
    for (int dt = 0; dt < 2; dt++) if (c->b_one_seen[dt]) { rc = batch_timings(c, dt); if (rc) return rc; }
    c->b_have_timings = 1;
  }
  bool gave_up = false;
  for (int dt = 1; dt >= 0; dt--) {
    const OnePlan& q = pl[dt];
    for (size_t j = 0; j < q.idx.size(); j++) {
      const int i = q.idx[j];
      const BatchResC& r = res[q.item_off + j];
      const bool in_place = false;                   // (such arrays are not in this launch)
      if (r.error == ONE_ERR_TIMEOUT) { gave_up = true; continue; }
      if (r.error) return fail(c, DCTZHIP_E_INTERNAL, "array %d: in-kernel error flag set (code %u)", i, r.error);
      double true_sf;
      if (!device_sf_stands(dt, r.stats[0], r.stats[1], r.sf_used, r.fast_used, &true_sf)) {   // (a table bug: never seen; the array is done again by the chain)
        if (in_place) return fail(c, DCTZHIP_E_INTERNAL, "array %d: scaling factor chosen on the device differs from the host's after an in-place pass", i);
        c->one = 0;
        continue;
      }
      done[i] = 1;
      if (!infos) continue;
      const HostStats st = {r.stats[0], r.stats[1], r.stats[2]};
      fill_cinfo(&infos[i], dt, mode, true_sf, st, items[i].n, r.cnt, (unsigned)((items[i].n + 63) / 64), DCTZHIP_INFO_STATS_FUSED | DCTZHIP_INFO_ONE_LAUNCH,
                 resq_h[q.item_off + j].qraw, r.q0);
    }
  }
  if (gave_up) { rc = one_gave_up(c); c->one_bdirty[0] = c->one_bdirty[1] = (unsigned)c->one_bctl_cap; if (rc) return rc; }
  return DCTZHIP_OK;
}

template <typename T>
static int fill_one_recs_d(dctzhip_ctx* c, const dctzhip_batch_ditem* items, const OnePlan& pl, OneRecD* recs, int mode, unsigned char* qt_host,
                           const unsigned char* qt_dev) {
  unsigned base = 0;
  size_t at = 0;
  for (size_t j = 0; j < pl.idx.size(); j++) {
    const dctzhip_batch_ditem& it = items[pl.idx[j]];
    OneRecD r;
    memset(&r, 0, sizeof(r));
    r.bin = it.d_bin_index; r.dc = it.d_dc; r.ac = it.d_ac_exact; r.out = it.d_out;
    r.nfull = (unsigned)(it.n / 64); r.rem = (unsigned)(it.n % 64); r.ntiles = (r.nfull + TILE_BLKS - 1) / TILE_BLKS;
    r.ac_count = it.ac_count;
    if (r.rem) { const T* rt = nullptr; int rc = rtab_for<T>(c, (int)r.rem, &rt); if (rc) return rc; r.rtab = rt; }
    if (mode == DCTZHIP_QT) {
      memcpy(qt_host + (pl.item_off + j) * 64 * sizeof(double), it.qtable_host, sizeof(T) * 64);
      r.qtab = qt_dev + (pl.item_off + j) * 64 * sizeof(double);
    }
    r.sf = (double)(T)it.sf;
    set_quant(r, inv_quant<T>(it.error_bound));
    r.eb = it.error_bound;
    r.nwg = pl.nwg[j]; r.board_base = base; r.item = (unsigned)(pl.item_off + j);
    for (unsigned w = 0; w < pl.nwg[j]; w++) { r.wg_local = w; recs[at++] = r; }
    base += pl.nwg[j];
  }
  return DCTZHIP_OK;
}

static int batch_one_decompress(dctzhip_ctx* c, int k, const dctzhip_batch_ditem* items, int mode, int* status, std::vector<char>& done, int* worst) {
  c->b_one_seen[0] = c->b_one_seen[1] = 0;
  if (!c->one || !c->handoff) return DCTZHIP_OK;
  if (c->one_cooldown > 0) { c->one_cooldown--; return DCTZHIP_OK; }
  OnePlan pl[2];
  size_t K = 0, nrec = 0;
  for (int dt = 1; dt >= 0; dt--) {
    OnePlan& q = pl[dt];
    for (int i = 0; i < k; i++) {
      if (items[i].dtype != dt || items[i].n >= BATCH_BIG) continue;
      q.idx.push_back(i); q.nwg.push_back(one_wgs_of(items[i].n)); q.grid += q.nwg.back();
    }
    const unsigned cap = dt == DCTZHIP_F64 ? one_capacity<double>(c, true, mode, false) : one_capacity<float>(c, true, mode, false);
    if (q.idx.empty() || q.grid > cap || q.grid > (unsigned)ONE_BOARD) { q.idx.clear(); q.nwg.clear(); q.grid = 0; continue; }
    q.item_off = K; K += q.idx.size();
    q.rec_off = nrec; nrec += q.grid;
  }
  if (K == 0) return DCTZHIP_OK;
  const size_t qt_off = (nrec * sizeof(OneRecD) + 255) & ~(size_t)255;
  const size_t blob = qt_off + (mode == DCTZHIP_QT ? K * 64 * sizeof(double) : 0);
  int rc = ensure_batch(c, K, blob, 0);
  if (rc) return rc;
  rc = ensure_batch(c, K, blob, c->b_cap * sizeof(BatchResD));
  if (rc) return rc;
  rc = ensure_one_bctl(c, K);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const unsigned tag = (unsigned)(++c->seq) | 0x80000000u;
  BatchResD* res = reinterpret_cast<BatchResD*>(c->b_res);
  for (size_t i = 0; i < K; i++) res[i].tag = 0;
  OneRecD* recs = reinterpret_cast<OneRecD*>(c->b_blob);
  for (int dt = 1; dt >= 0; dt--) {
    if (pl[dt].idx.empty()) continue;
    rc = dt == DCTZHIP_F64 ? fill_one_recs_d<double>(c, items, pl[dt], recs + pl[dt].rec_off, mode, c->b_blob + qt_off, c->b_blob_hdev + qt_off)
                           : fill_one_recs_d<float>(c, items, pl[dt], recs + pl[dt].rec_off, mode, c->b_blob + qt_off, c->b_blob_hdev + qt_off);
    if (rc) return rc;
  }
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  for (int dt = 1; dt >= 0; dt--) {
    const OnePlan& q = pl[dt];
    if (q.idx.empty()) continue;
    const unsigned epoch = one_next_epoch(c);
    if (!epoch) { (void)one_gave_up(c); return DCTZHIP_E_HIP; }
    const bool prof = c->profiling != 0;
    hipEvent_t* ev = c->b_ev[dt];
    if (prof) { for (int i = 0; i < 5; i++) if (!ev[i]) HIPCHK(c, hipEventCreate(&ev[i])); HIPCHK(c, hipEventRecord(ev[0], s)); HIPCHK(c, hipEventRecord(ev[1], s)); }
    OneBoard b;
    b.ga = c->one_ga; b.gb = c->one_gb; b.rec = c->one_rec; b.epoch = epoch; b.nwg = 0; b.dbg = nullptr;
    const OneRecD* recs_d = reinterpret_cast<const OneRecD*>(c->b_blob_hdev) + q.rec_off;
    // (decode only ever sets `error` in its control block: any of this context's blocks will do)
    if (dt == DCTZHIP_F64) {
      OneBatchD<double> cm = {recs_d, c->tab_f64, c->one_bctl, b, reinterpret_cast<BatchResD*>(c->b_res_hdev), tag, c->one_withhold ? 1u : 0u};
      launch_decompress_one_batch<double>(cm, q.grid, mode, s);
      SET_LAST(c, 4, "k_decompress_one_batch<double, %d>", mode);
    } else {
      OneBatchD<float> cm = {recs_d, c->tab_f32, c->one_bctl, b, reinterpret_cast<BatchResD*>(c->b_res_hdev), tag, c->one_withhold ? 1u : 0u};
      launch_decompress_one_batch<float>(cm, q.grid, mode, s);
      SET_LAST(c, 5, "k_decompress_one_batch<float, %d>", mode);
    }
    if (prof) { HIPCHK(c, hipEventRecord(ev[2], s)); HIPCHK(c, hipEventRecord(ev[3], s)); HIPCHK(c, hipEventRecord(ev[4], s)); }
    HIPCHK(c, hipGetLastError());
    c->one_calls++;
    c->b_one_seen[dt] = 1;
  }
  rc = wait_tags(c, &res[0].tag, sizeof(BatchResD), K, tag, "decompress batch (one launch)");
  if (rc) { (void)one_gave_up(c); return rc; }
  if (c->profiling) {
    c->b_last[0] = dctzhip_timings{0, 0, 0, 0}; c->b_last[1] = dctzhip_timings{0, 0, 0, 0};
    for (int dt = 0; dt < 2; dt++) if (c->b_one_seen[dt]) { rc = batch_timings(c, dt); if (rc) return rc; }
    c->b_have_timings = 1;
  }
  bool gave_up = false;
  for (int dt = 1; dt >= 0; dt--) {
    const OnePlan& q = pl[dt];
    for (size_t j = 0; j < q.idx.size(); j++) {
      const int i = q.idx[j];
      const BatchResD& r = res[q.item_off + j];
      if (r.error == ONE_ERR_TIMEOUT) { gave_up = true; continue; }
      done[i] = 1;
      if (r.error == 2) {
        *worst = DCTZHIP_E_ARG;
        if (status) status[i] = DCTZHIP_E_ARG;
        fail(c, DCTZHIP_E_ARG, "array %d: bin_index flags more exact coefficients than ac_count provides", i);
      } else if (r.error) return fail(c, DCTZHIP_E_INTERNAL, "array %d: in-kernel error flag set (code %u)", i, r.error);
    }
  }
  if (gave_up) { c->one_bdirty[0] = c->one_bdirty[1] = (unsigned)c->one_bctl_cap; rc = one_gave_up(c); if (rc) return rc; }
  return DCTZHIP_OK;
}

extern "C" int dctzhip_compress_batch(dctzhip_ctx* c, int k, const dctzhip_batch_citem* items_in, int mode, dctzhip_cinfo* infos) {
  const dctzhip_batch_citem* items = items_in;
  if (!c) return DCTZHIP_E_ARG;
  if (k < 0 || (k && !items)) return fail(c, DCTZHIP_E_ARG, "dctzhip_compress_batch: bad arguments");
  if (k == 0) return DCTZHIP_OK;
  for (int i = 0; i < k; i++) {
    const dctzhip_batch_citem& it = items[i];
    int rc = check_common(c, it.n, it.dtype, mode);
    if (rc) return rc;
    if (!it.d_in || !it.d_bin_index || !it.d_dc || !it.d_ac_exact) return fail(c, DCTZHIP_E_ARG, "array %d: null device buffer", i);
    if (!aligned16(it.d_in) || !aligned16(it.d_bin_index) || !aligned16(it.d_dc) || !aligned16(it.d_ac_exact) || (it.d_scaled && !aligned16(it.d_scaled)))
      return fail(c, DCTZHIP_E_ARG, "array %d: device buffers must be 16-byte aligned", i);
    if (it.error_bound < 1E-6) return fail(c, DCTZHIP_E_BOUND, "array %d: ERROR BOUND is not acceptable", i);   // dctz-comp-lib.c:135-138
  }
  // Every item compresses its input as it was when the call was made.  An item that scales its input in place while another
  // item reads those bytes -- in another sequence, on the other chain, on the single-array path or in a redo -- is planned
  // as a reader (no scaled copy) and its division runs at the very end, behind every read of the call.
  std::vector<char> deferred((size_t)k, 0);
  bool any_deferred = false;
  {
    std::vector<Span> sp(5 * (size_t)k);
    size_t m = 0;
    for (int i = 0; i < k; i++) {
      const dctzhip_batch_citem& it = items[i];
      compress_spans(sp.data(), &m, i, it.d_in, it.n, it.dtype, it.d_bin_index, it.d_dc, it.d_ac_exact, it.d_scaled, nullptr);
    }
    int rc = check_spans(c, sp.data(), m, "dctzhip_compress_batch", deferred.data());
    if (rc) return rc;
    for (int i = 0; i < k; i++) any_deferred = any_deferred || deferred[i];
  }
  std::vector<dctzhip_batch_citem> planned;
  std::vector<dctzhip_cinfo> own_infos;
  if (any_deferred) {
    planned.assign(items_in, items_in + k);
    for (int i = 0; i < k; i++) if (deferred[i]) planned[i].d_scaled = nullptr;
    items = planned.data();
    if (!infos) { own_infos.resize((size_t)k); infos = own_infos.data(); }     // (the deferred divisions need the sf)
  }
  HIPCHK(c, hipSetDevice(c->device));
  const bool box = c->handoff != 0 && c->dev_sf && c->sf_nk[0] > 0 && c->sf_nk[1] > 0;
  // arrays whose workgroups all fit the chip at once: one launch per element type (dctz_kernels_one.hip)
  std::vector<char> done((size_t)k, 0);
  { int rc = batch_one_compress(c, k, items, mode, infos, done); if (rc) return rc; }
  // arrays that gain nothing from a batch (launch cost is noise beside their kernels, and the single-array path saves
  // them the statistics pass) -- and every array when the platform has no mailbox -- take the single-array path
  std::vector<int> single;
  std::vector<SeqC> seqs;
  for (int dt = 1; dt >= 0; dt--) {                   // fp64 sequences first, then fp32
    SeqC cur; cur.dtype = dt;
    for (int i = 0; i < k; i++) {
      if (items[i].dtype != dt || done[i]) continue;
      if (!box || items[i].n >= BATCH_BIG) { if (dt == items[i].dtype) single.push_back(i); continue; }
      cur.idx.push_back(i);
      if ((int)cur.idx.size() == BATCH_MAX) { seqs.push_back(cur); cur = SeqC(); cur.dtype = dt; }
    }
    if (!cur.idx.empty()) seqs.push_back(cur);
  }
  size_t K = 0, blob = 0;
  bool has[2] = {false, false};
  for (const SeqC& q : seqs) has[q.dtype] = true;
  const bool two = has[0] && has[1];                   // mixed batch: the fp32 sequences run beside the fp64 ones
  size_t tiles_max[2] = {0, 0}, lists_max[2] = {0, 0};
  Chain ch[2];
  c->b_spec_now = c->spec_cooldown == 0;               // (a wrong guess pauses the speculation of the next calls, batches included)
  if (!c->b_spec_now && !seqs.empty()) c->spec_cooldown--;
  for (size_t qi = 0; qi < seqs.size(); qi++) {
    SeqC& q = seqs[qi];
    q.chain = (two && q.dtype == DCTZHIP_F32) ? 1 : 0;
    if (q.dtype == DCTZHIP_F64) plan_compress<double>(c, items, mode, q, two ? 2u : 1u); else plan_compress<float>(c, items, mode, q, two ? 2u : 1u);
    q.item_off = K; K += q.idx.size();
    q.blob_off = blob; blob += q.blob_bytes;
    if (q.tiles_total > tiles_max[q.chain]) tiles_max[q.chain] = q.tiles_total;
    if (q.lists_total > lists_max[q.chain]) lists_max[q.chain] = q.lists_total;
    ch[q.chain].last = (int)qi;
  }
  if (!seqs.empty()) {
    // scratch: one region per chain, sized for the chain's largest sequence (its sequences follow each other on the
    // chain's stream and reuse it), in the widest element type
    ch[1].tile_off = tiles_max[0]; ch[1].list_off = lists_max[0] + 2; ch[1].part_off = PART_SLOTS;
    int rc = ensure_scratch(c, (tiles_max[0] + tiles_max[1]) * TILE_ELEMS, DCTZHIP_F64, mode, true, lists_max[0] + lists_max[1] + 6);
    if (rc) return rc;
    rc = ensure_batch(c, K, blob, 0);
    if (rc) return rc;
    rc = ensure_batch(c, K, blob, c->b_cap * (sizeof(BatchResC) + (mode == DCTZHIP_QT ? sizeof(BatchResQ) : 0)));
    if (rc) return rc;
    rc = chains_fork(c, ch, two);
    if (rc) return rc;
    const unsigned long long seq = ++c->seq;
    bool seen[2] = {false, false};
    // (from here on every exit joins the second stream first: its kernels share this context's scratch with whatever the
    // next call queues on the first one)
    auto bail = [&](int code) { (void)chains_join(c, two); c->ctl_dirty = 1; c->b_ctl_dirty = 1; return code; };
    for (size_t qi = 0; qi < seqs.size(); qi++) {
      const SeqC& q = seqs[qi];
      const bool last = ch[q.chain].last == (int)qi;
      rc = (q.dtype == DCTZHIP_F64) ? launch_compress_seq<double>(c, items, mode, q, ch[q.chain], last, seq, !seen[q.dtype])
                                    : launch_compress_seq<float>(c, items, mode, q, ch[q.chain], last, seq, !seen[q.dtype]);
      if (rc) return bail(rc);
      seen[q.dtype] = true;
    }
    rc = chains_join(c, two);
    if (rc) return rc;
    rc = wait_seq(c, ch[0].word, seq, "compress batch");
    if (rc) { c->b_ctl_dirty = 1; return rc; }
    if (two) { rc = wait_seq(c, ch[1].word, seq, "compress batch (second chain)"); if (rc) { c->b_ctl_dirty = 1; return rc; } }
    if (c->profiling) {
      for (int dt = 0; dt < 2; dt++) if (!c->b_one_seen[dt]) c->b_last[dt] = dctzhip_timings{0, 0, 0, 0};
      for (int dt = 0; dt < 2; dt++) if (seen[dt]) { rc = batch_timings(c, dt); if (rc) return rc; }
      c->b_have_timings = 1;
    }
    // results; the device's choice of every scaling factor against the host's own expression (util.c:29 / :43)
    const BatchResC* res = reinterpret_cast<const BatchResC*>(c->b_res);
    const BatchResQ* resq = reinterpret_cast<const BatchResQ*>(c->b_res + c->b_cap * sizeof(BatchResC));
    for (const SeqC& q : seqs) {
      for (size_t j = 0; j < q.idx.size(); j++) {
        const int i = q.idx[j];
        const BatchResC& r = res[q.item_off + j];
        const int dtype = q.dtype;
        double true_sf;
        const bool stands = device_sf_stands(dtype, r.stats[0], r.stats[1], r.sf_used, r.fast_used, &true_sf);
        if (q.sample[j]) c->b_spec_items++;
        if (!stands) {                                // (a speculative item whose sample missed the decade; else a table bug: never seen): done again on its own
          if (q.sample[j]) { c->b_spec_misses++; c->spec_misses++; c->spec_cooldown = SPEC_COOLDOWN; }
          // ... unless k_scale_batch has already divided the input in place by the wrong factor: nothing to run it on again
          if (items[i].d_scaled && items[i].d_scaled == items[i].d_in)
            return fail(c, DCTZHIP_E_INTERNAL, "array %d: scaling factor %g chosen on the device differs from the host's %g after an in-place pass", i, r.sf_used, true_sf);
          single.push_back(i);
          continue;
        }
        if (!infos) continue;
        dctzhip_cinfo* info = &infos[i];
        memset(info, 0, sizeof(*info));
        const size_t n = items[i].n;
        info->sf = true_sf;
        info->mean = (dtype == DCTZHIP_F64) ? r.stats[2] / (double)(int)n : (double)((float)r.stats[2] / (float)(int)n);
        info->max_abs = r.stats[0]; info->min_abs = r.stats[1];
        info->cnt = r.cnt; info->nblk = (uint32_t)((n + 63) / 64);
        if (q.sample[j]) info->flags |= DCTZHIP_INFO_STATS_FUSED;
        if (mode == DCTZHIP_QT) {
          const BatchResQ& rq = resq[q.item_off + j];
          for (int jj = 0; jj < 64; jj++) {
            double v;
            if (dtype == DCTZHIP_F64) { unsigned long long b = rq.qraw[jj]; memcpy(&v, &b, 8); }
            else { unsigned int b = (unsigned int)rq.qraw[jj]; float f; memcpy(&f, &b, 4); v = f; }
            info->qtable_raw[jj] = v;
            info->qtable[jj] = (jj >= 1 && v < 1.0) ? 1.0 : v;          // :450-461
          }
          double q0;
          if (dtype == DCTZHIP_F64) { unsigned long long b = r.q0; memcpy(&q0, &b, 8); }
          else { unsigned int b = (unsigned int)r.q0; float f; memcpy(&f, &b, 4); q0 = f; }
          info->qtable[0] = info->qtable_raw[0] = q0;                 // :355-360
        }
      }
    }
  }
  for (int i : single) {
    const dctzhip_batch_citem& it = items[i];
    int rc = dctzhip_compress(c, it.d_in, it.n, it.dtype, it.error_bound, mode, it.d_bin_index, it.d_dc, it.d_ac_exact, it.d_scaled, nullptr,
                              infos ? &infos[i] : nullptr);
    if (rc) return rc;
  }
  // the deferred in-place divisions, on the context's stream behind both chains and every single-array call (k_scale: the
  // division of k_scale_batch, dctz-comp-lib.c:193-216)
  for (int i = 0; i < k && any_deferred; i++) {
    if (!deferred[i]) continue;
    const dctzhip_batch_citem& it = items_in[i];
    const double sf = infos[i].sf;
    if (it.dtype == DCTZHIP_F64) { if (sf != 1.0) launch_scale<double>((const double*)it.d_in, (double*)it.d_scaled, it.n, sf, c->num_cu * 8, c->stream); }
    else if ((float)sf != 1.0f) launch_scale<float>((const float*)it.d_in, (float*)it.d_scaled, it.n, (float)sf, c->num_cu * 8, c->stream);
  }
  if (any_deferred) HIPCHK(c, hipGetLastError());
  if (c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

// ---- decode side of a batch ----
template <typename T>
static void plan_decompress(dctzhip_ctx* c, const dctzhip_batch_ditem* items, int mode, SeqD& q, unsigned cap_div) {
  const size_t k = q.idx.size();
  unsigned cap = (unsigned)(c->num_cu * wg_per_cu<T>(c, true, mode, false, GEOM_1D)) / cap_div;
  cap = cap > 2 * (unsigned)k ? cap - (unsigned)k : cap / 2 + 1;
  size_t tiles = 0;
  q.nfull.resize(k); q.rem.resize(k); q.ntiles.resize(k); q.nwg.resize(k); q.tile_base.resize(k); q.wg_base.resize(k);
  for (size_t j = 0; j < k; j++) {
    const size_t n = items[q.idx[j]].n;
    q.nfull[j] = (unsigned)(n / 64); q.rem[j] = (unsigned)(n % 64);
    q.ntiles[j] = (q.nfull[j] + TILE_BLKS - 1) / TILE_BLKS;
    tiles += q.ntiles[j];
  }
  for (size_t j = 0; j < k; j++) {
    q.nwg[j] = share_of(q.ntiles[j], tiles, cap);
    q.tile_base[j] = (unsigned)q.tiles_total; q.tiles_total += q.ntiles[j];
    q.wg_base[j] = (unsigned)q.wgs_total; q.wgs_total += q.nwg[j];
    q.grid_main += q.nwg[j];
    q.grid_cnt += q.nwg[j] ? q.nwg[j] : 1u;
    q.nrem += q.rem[j] ? 1u : 0u;
  }
  q.blob_bytes = align16(k * sizeof(BatchInv<T>)) + align16(2 * (k + 1) * sizeof(unsigned) + (size_t)q.nrem * sizeof(unsigned));
}

template <typename T>
static int launch_decompress_seq(dctzhip_ctx* c, const dctzhip_batch_ditem* items, int mode, const SeqD& q, const Chain& ch, bool publish,
                                 unsigned long long seq, bool first_of_dtype) {
  const int dtype = sizeof(T) == 8 ? DCTZHIP_F64 : DCTZHIP_F32;
  const size_t k = q.idx.size();
  hipStream_t s = ch.s;
  if (ch.tile_off + q.tiles_total + 2 > c->tile_cap || ch.list_off + q.wgs_total + 2 > c->tile_cap)
    return fail(c, DCTZHIP_E_INTERNAL, "batch: scratch plan exceeds its buffers");
  unsigned char* hb = c->b_blob + q.blob_off;
  BatchInv<T>* hi = reinterpret_cast<BatchInv<T>*>(hb);
  const size_t first_off = align16(k * sizeof(BatchInv<T>));
  unsigned* f_cnt = reinterpret_cast<unsigned*>(hb + first_off), *f_main = f_cnt + (k + 1), *rem_items = f_cnt + 2 * (k + 1);
  unsigned char* db = c->b_blob_dev + q.blob_off;
  unsigned a_cnt = 0, a_main = 0, nrem = 0;
  for (size_t j = 0; j < k; j++) {
    const dctzhip_batch_ditem& it = items[q.idx[j]];
    BatchInv<T>& b = hi[j];
    memset(&b, 0, sizeof(b));
    InvParams<T>& p = b.p;
    p.bin = (const uint8_t*)it.d_bin_index; p.dc = it.d_dc; p.ac = it.d_ac_exact; p.out = (T*)it.d_out;
    p.tab = tab_of<T>(c); p.rtab = nullptr;
    if (q.rem[j]) { int rc = rtab_for<T>(c, (int)q.rem[j], &p.rtab); if (rc) return rc; }
    p.qtab = reinterpret_cast<const T*>(db + j * sizeof(BatchInv<T>) + offsetof(BatchInv<T>, qtab));
    if (mode == DCTZHIP_QT) memcpy(b.qtab, it.qtable_host, sizeof(T) * 64);
    p.tile_cnt = c->tile_cnt + ch.tile_off + q.tile_base[j]; p.wg_cnt = c->wg_cnt + ch.list_off + q.wg_base[j]; p.tile_pre = nullptr;
    p.ctl = c->b_ctl + q.item_off + j;
    p.nfull = q.nfull[j]; p.ntiles = q.ntiles[j]; p.ac_count = it.ac_count; p.nwg = q.nwg[j];
    p.sf = (T)it.sf;
    set_quant(p, inv_quant<T>(it.error_bound));
    p.eb = it.error_bound;
    b.n = (unsigned)it.n; b.rem = q.rem[j]; b.scale = (p.sf != (T)1.0) ? 1u : 0u; b.cnt_wgs = q.nwg[j] ? q.nwg[j] : 1u;
    b.rem_cnt = c->b_remcnt + q.item_off + j;
    f_cnt[j] = a_cnt; a_cnt += b.cnt_wgs;
    f_main[j] = a_main; a_main += q.nwg[j];
    if (q.rem[j]) rem_items[nrem++] = (unsigned)j;
  }
  f_cnt[k] = a_cnt; f_main[k] = a_main;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  const BatchInv<T>* it_h = reinterpret_cast<const BatchInv<T>*>(c->b_blob_hdev + q.blob_off);
  const unsigned* first_h = reinterpret_cast<const unsigned*>(c->b_blob_hdev + q.blob_off + first_off);
  const BatchInv<T>* it_d = reinterpret_cast<const BatchInv<T>*>(db);
  const unsigned* first_d = reinterpret_cast<const unsigned*>(db + first_off);
  const bool prof = c->profiling && first_of_dtype;
  hipEvent_t* ev = c->b_ev[dtype];
  if (prof) for (int i = 0; i < 5; i++) if (!ev[i]) HIPCHK(c, hipEventCreate(&ev[i]));
  if (prof) HIPCHK(c, hipEventRecord(ev[0], s));
  launch_count_batch<T>(it_h, first_h, (unsigned)k, q.grid_cnt, c->b_blob_hdev + q.blob_off, db, q.blob_bytes, s);
  if (prof) HIPCHK(c, hipEventRecord(ev[1], s));
  BatchFin fin;
  fin.word = publish ? const_cast<unsigned long long*>(ch.word_dev) : nullptr; fin.seq = seq;
  fin.res = c->b_res_hdev + q.item_off * sizeof(BatchResD); fin.resq = nullptr;
  if (q.grid_main) { launch_decompress_batch<T>(it_d, first_d + (k + 1), (unsigned)k, q.grid_main, mode, fin, s); SET_LAST(c, sizeof(T) == 8 ? 4 : 5, "k_decompress_batch<%s, %d>", tname<T>(), mode); }
  if (prof) HIPCHK(c, hipEventRecord(ev[2], s));
  if (nrem) launch_decompress_rem_batch<T>(it_d, first_d + 2 * (k + 1), nrem, mode, s);
  if (prof) { HIPCHK(c, hipEventRecord(ev[3], s)); HIPCHK(c, hipEventRecord(ev[4], s)); }
  HIPCHK(c, hipGetLastError());
  return DCTZHIP_OK;
}

extern "C" int dctzhip_decompress_batch(dctzhip_ctx* c, int k, const dctzhip_batch_ditem* items, int mode, int* status) {
  if (!c) return DCTZHIP_E_ARG;
  if (k < 0 || (k && !items)) return fail(c, DCTZHIP_E_ARG, "dctzhip_decompress_batch: bad arguments");
  if (k == 0) return DCTZHIP_OK;
  for (int i = 0; i < k; i++) {
    const dctzhip_batch_ditem& it = items[i];
    int rc = check_common(c, it.n, it.dtype, mode);
    if (rc) return rc;
    if (!it.d_bin_index || !it.d_dc || !it.d_out || (it.ac_count && !it.d_ac_exact)) return fail(c, DCTZHIP_E_ARG, "array %d: null device buffer", i);
    if (!aligned16(it.d_bin_index) || !aligned16(it.d_out)) return fail(c, DCTZHIP_E_ARG, "array %d: device buffers must be 16-byte aligned", i);
    if (((uintptr_t)it.d_dc & 3u) || ((uintptr_t)it.d_ac_exact & 3u)) return fail(c, DCTZHIP_E_ARG, "array %d: DC and AC_exact must be 4-byte aligned", i);
    if (mode == DCTZHIP_QT && !it.qtable_host) return fail(c, DCTZHIP_E_ARG, "array %d: QT mode needs the 64-entry table", i);
    if (status) status[i] = DCTZHIP_OK;
  }
  {
    std::vector<Span> sp(4 * (size_t)k);
    size_t m = 0;
    for (int i = 0; i < k; i++)
      decompress_spans(sp.data(), &m, i, items[i].d_bin_index, items[i].d_dc, items[i].d_ac_exact, items[i].ac_count, items[i].n, items[i].dtype, items[i].d_out);
    int rc = check_spans(c, sp.data(), m, "dctzhip_decompress_batch", nullptr);
    if (rc) return rc;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const bool box = c->handoff != 0;
  int worst = DCTZHIP_OK;
  std::vector<char> done((size_t)k, 0);
  { int rc = batch_one_decompress(c, k, items, mode, status, done, &worst); if (rc) return rc; }
  std::vector<int> single;
  std::vector<SeqD> seqs;
  for (int dt = 1; dt >= 0; dt--) {
    SeqD cur; cur.dtype = dt;
    for (int i = 0; i < k; i++) {
      if (items[i].dtype != dt || done[i]) continue;
      // (an array with tiles but no mailbox, or without any full tile, keeps the single-array path: the batch hands off in
      // the first workgroup of k_decompress_batch)
      if (!box || items[i].n >= BATCH_BIG) { single.push_back(i); continue; }
      cur.idx.push_back(i);
      if ((int)cur.idx.size() == BATCH_MAX) { seqs.push_back(cur); cur = SeqD(); cur.dtype = dt; }
    }
    if (!cur.idx.empty()) seqs.push_back(cur);
  }
  size_t K = 0, blob = 0;
  // a sequence whose arrays have no full tile at all has no k_decompress_batch launch to hand off from: single path
  // (planned once to find out: the grid does not depend on the chains)
  for (size_t qi = 0; qi < seqs.size();) {
    SeqD probe = seqs[qi];
    if (probe.dtype == DCTZHIP_F64) plan_decompress<double>(c, items, mode, probe, 1u); else plan_decompress<float>(c, items, mode, probe, 1u);
    if (probe.grid_main == 0) { for (int i : seqs[qi].idx) single.push_back(i); seqs.erase(seqs.begin() + qi); } else qi++;
  }
  bool has[2] = {false, false};
  for (const SeqD& q : seqs) has[q.dtype] = true;
  const bool two = has[0] && has[1];
  size_t tiles_max[2] = {0, 0}, wgs_max[2] = {0, 0};
  Chain ch[2];
  for (size_t qi = 0; qi < seqs.size(); qi++) {
    SeqD& q = seqs[qi];
    q.chain = (two && q.dtype == DCTZHIP_F32) ? 1 : 0;
    if (q.dtype == DCTZHIP_F64) plan_decompress<double>(c, items, mode, q, two ? 2u : 1u); else plan_decompress<float>(c, items, mode, q, two ? 2u : 1u);
    q.item_off = K; K += q.idx.size();
    q.blob_off = blob; blob += q.blob_bytes;
    if (q.tiles_total > tiles_max[q.chain]) tiles_max[q.chain] = q.tiles_total;
    if (q.wgs_total > wgs_max[q.chain]) wgs_max[q.chain] = q.wgs_total;
    ch[q.chain].last = (int)qi;
  }
  if (!seqs.empty()) {
    ch[1].tile_off = tiles_max[0] + 2; ch[1].list_off = wgs_max[0] + 2;
    int rc = ensure_scratch(c, (tiles_max[0] + tiles_max[1] + 6) * TILE_ELEMS, DCTZHIP_F64, DCTZHIP_EC, false, wgs_max[0] + wgs_max[1] + 6);
    if (rc) return rc;
    rc = ensure_batch(c, K, blob, 0);
    if (rc) return rc;
    rc = ensure_batch(c, K, blob, c->b_cap * sizeof(BatchResD));
    if (rc) return rc;
    if (c->b_ctl_dirty) { HIPCHK(c, hipMemsetAsync(c->b_ctl, 0, c->b_cap * sizeof(Ctl), c->stream)); c->b_ctl_dirty = 0; }
    rc = chains_fork(c, ch, two);
    if (rc) return rc;
    const unsigned long long seq = ++c->seq;
    bool seen[2] = {false, false};
    auto bail = [&](int code) { (void)chains_join(c, two); c->ctl_dirty = 1; c->b_ctl_dirty = 1; return code; };   // (as in dctzhip_compress_batch)
    for (size_t qi = 0; qi < seqs.size(); qi++) {
      const SeqD& q = seqs[qi];
      const bool last = ch[q.chain].last == (int)qi;
      rc = (q.dtype == DCTZHIP_F64) ? launch_decompress_seq<double>(c, items, mode, q, ch[q.chain], last, seq, !seen[q.dtype])
                                    : launch_decompress_seq<float>(c, items, mode, q, ch[q.chain], last, seq, !seen[q.dtype]);
      if (rc) return bail(rc);
      seen[q.dtype] = true;
    }
    rc = chains_join(c, two);
    if (rc) return rc;
    rc = wait_seq(c, ch[0].word, seq, "decompress batch");
    if (rc) { c->b_ctl_dirty = 1; return rc; }
    if (two) { rc = wait_seq(c, ch[1].word, seq, "decompress batch (second chain)"); if (rc) { c->b_ctl_dirty = 1; return rc; } }
    if (c->profiling) {
      for (int dt = 0; dt < 2; dt++) if (!c->b_one_seen[dt]) c->b_last[dt] = dctzhip_timings{0, 0, 0, 0};
      for (int dt = 0; dt < 2; dt++) if (seen[dt]) { rc = batch_timings(c, dt); if (rc) return rc; }
      c->b_have_timings = 1;
    }
    const BatchResD* res = reinterpret_cast<const BatchResD*>(c->b_res);
    for (const SeqD& q : seqs)
      for (size_t j = 0; j < q.idx.size(); j++)
        if (res[q.item_off + j].error) {
          c->b_ctl_dirty = 1;
          worst = DCTZHIP_E_ARG;
          if (status) status[q.idx[j]] = DCTZHIP_E_ARG;
          fail(c, DCTZHIP_E_ARG, "array %d: bin_index flags more exact coefficients than ac_count provides", q.idx[j]);
        }
  }
  for (int i : single) {
    const dctzhip_batch_ditem& it = items[i];
    int rc = dctzhip_decompress(c, it.d_bin_index, it.d_dc, it.d_ac_exact, it.ac_count, it.qtable_host, it.n, it.dtype, it.error_bound, it.sf, mode,
                                it.d_out);
    if (rc == DCTZHIP_E_ARG) { worst = rc; if (status) status[i] = rc; continue; }
    if (rc) return rc;
  }
  if (worst == DCTZHIP_OK && c->blocking) HIPCHK(c, hipStreamSynchronize(c->stream));
  return worst;
}

// ---- multi-GPU gather over RCCL -----------------------------------------------------------------------------------
// The few RCCL entry points used, resolved with dlopen so that libdctzhip.so itself has no RCCL dependency.
namespace {
struct rccl_id { char internal[DCTZHIP_COMM_ID_BYTES]; };
struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(rccl_id*) = nullptr;
  int (*CommInitRank)(void**, int, rccl_id, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
Rccl g_rccl;
// ncclDataType_t as /opt/rocm/include/rccl/rccl.h spells it: ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3,
// ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclFloat32 = 7, ncclFloat64 = 8 (the library is loaded with dlopen, so
// the header is not included; tests/test_abi_cpu.py compares these three with the header's text when it is installed)
constexpr int NCCL_UINT8 = DCTZ_NCCL_UINT8, NCCL_UINT64 = DCTZ_NCCL_UINT64, NCCL_FLOAT32 = DCTZ_NCCL_FLOAT32;
constexpr int RCCL_MAJOR_KNOWN = 2;                  // ncclGetVersion() / 10000 this file's call signatures were read from

bool rccl_load(dctzhip_ctx* c) {
  if (g_rccl.ok) return true;
  // DCTZHIP_RCCL_LIBRARY: an RCCL build outside the loader's path -- or the test double of tests/c/rccl_double.cpp
  const char* names[] = {getenv("DCTZHIP_RCCL_LIBRARY"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) {
    if (!n || !*n) continue;
    g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (g_rccl.h || n == names[0]) break;            // (a library that was asked for by name is not silently replaced)
  }
  if (!g_rccl.h) { fail(c, DCTZHIP_E_HIP, "RCCL not found (dlopen %s): %s", names[0] && *names[0] ? names[0] : "librccl.so", dlerror()); return false; }
#define SYM(field, name) *(void**)(&g_rccl.field) = dlsym(g_rccl.h, name); if (!g_rccl.field) { fail(c, DCTZHIP_E_HIP, "RCCL symbol %s missing", name); return false; }
  SYM(GetUniqueId, "ncclGetUniqueId") SYM(CommInitRank, "ncclCommInitRank") SYM(CommDestroy, "ncclCommDestroy")
  SYM(AllGather, "ncclAllGather") SYM(Send, "ncclSend") SYM(Recv, "ncclRecv") SYM(GroupStart, "ncclGroupStart")
  SYM(GroupEnd, "ncclGroupEnd") SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
  // the by-value 128-byte id, the enum values and the argument lists above are those of NCCL 2.x: a library of another
  // major version is refused here, before the first call through a pointer of the wrong shape
  {
    int (*get_version)(int*) = nullptr;
    *(void**)(&get_version) = dlsym(g_rccl.h, "ncclGetVersion");
    int v = 0;
    if (!get_version || get_version(&v) != 0) { fail(c, DCTZHIP_E_HIP, "RCCL: ncclGetVersion is missing or failed"); return false; }
    const int major = v >= 10000 ? v / 10000 : v / 1000;        // (NCCL_VERSION: X * 10000 + Y * 100 + Z from 2.9 on, X * 1000 + ... before)
    if (major != RCCL_MAJOR_KNOWN) { fail(c, DCTZHIP_E_HIP, "RCCL version code %d (major %d): this library speaks the NCCL %d API only", v, major, RCCL_MAJOR_KNOWN); return false; }
  }
  g_rccl.ok = true;
  return true;
}
}  // namespace

#define RCCLCHK(c, call)                                                                                  \
  do {                                                                                                    \
    int r_ = (call);                                                                                      \
    if (r_ != 0) return fail((c), DCTZHIP_E_HIP, "%s failed: %s", #call, g_rccl.GetErrorString(r_));      \
  } while (0)

extern "C" int dctzhip_comm_unique_id(void* id_out) {
  if (!id_out) return fail(nullptr, DCTZHIP_E_ARG, "dctzhip_comm_unique_id: id_out is NULL");
  if (!rccl_load(nullptr)) return DCTZHIP_E_HIP;
  rccl_id id;
  RCCLCHK(nullptr, g_rccl.GetUniqueId(&id));
  memcpy(id_out, id.internal, DCTZHIP_COMM_ID_BYTES);
  return DCTZHIP_OK;
}

extern "C" int dctzhip_comm_create(dctzhip_ctx* c, int rank, int world, const void* id_in) {
  if (!c || !id_in) return DCTZHIP_E_ARG;
  if (world < 1 || rank < 0 || rank >= world) return fail(c, DCTZHIP_E_ARG, "rank %d of %d", rank, world);
  if (c->comm) return fail(c, DCTZHIP_E_ARG, "the context already has a communicator");
  if (!rccl_load(c)) return DCTZHIP_E_HIP;
  HIPCHK(c, hipSetDevice(c->device));
  rccl_id id;
  memcpy(id.internal, id_in, DCTZHIP_COMM_ID_BYTES);
  RCCLCHK(c, g_rccl.CommInitRank(&c->comm, world, id, rank));
  c->comm_rank = rank; c->comm_world = world;
  HIPCHK(c, hipMalloc(&c->comm_sizes_dev, sizeof(unsigned long long) * 3 * (size_t)(world + 1)));
  return DCTZHIP_OK;
}

extern "C" int dctzhip_comm_destroy(dctzhip_ctx* c) {
  if (!c) return DCTZHIP_E_ARG;
  if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
  if (c->comm_sizes_dev) { (void)hipFree(c->comm_sizes_dev); c->comm_sizes_dev = nullptr; }
  c->comm_world = 0;
  return DCTZHIP_OK;
}

extern "C" int dctzhip_comm_sizes(dctzhip_ctx* c, uint64_t n, uint64_t cnt, uint64_t* sizes) {
  if (!c || !sizes) return DCTZHIP_E_ARG;
  if (!c->comm) return fail(c, DCTZHIP_E_ARG, "dctzhip_comm_create was not called");
  HIPCHK(c, hipSetDevice(c->device));
  const int W = c->comm_world;
  unsigned long long mine[3] = {n, (n + 63) / 64, cnt};
  unsigned long long* d_mine = c->comm_sizes_dev + 3 * (size_t)W;
  HIPCHK(c, hipMemcpyAsync(d_mine, mine, sizeof(mine), hipMemcpyHostToDevice, c->stream));
  RCCLCHK(c, g_rccl.AllGather(d_mine, c->comm_sizes_dev, 3, NCCL_UINT64, c->comm, c->stream));
  HIPCHK(c, hipMemcpyAsync(sizes, c->comm_sizes_dev, sizeof(unsigned long long) * 3 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DCTZHIP_OK;
}

extern "C" int dctzhip_comm_gather(dctzhip_ctx* c, int root, const void* d_bin, const float* d_dc, const float* d_ac,
                                   const uint64_t* sizes, void* d_bin_all, float* d_dc_all, float* d_ac_all) {
  if (!c || !sizes) return DCTZHIP_E_ARG;
  if (!c->comm) return fail(c, DCTZHIP_E_ARG, "dctzhip_comm_create was not called");
  const int W = c->comm_world, me = c->comm_rank;
  if (root < 0 || root >= W) return fail(c, DCTZHIP_E_ARG, "root %d of %d", root, W);
  if (me == root && (!d_bin_all || !d_dc_all || (!d_ac_all && [&] { uint64_t t = 0; for (int r = 0; r < W; r++) t += sizes[3 * r + 2]; return t; }() > 0)))
    return fail(c, DCTZHIP_E_ARG, "the root needs the three receive buffers");
  if (!d_bin || !d_dc || (sizes[3 * me + 2] && !d_ac)) return fail(c, DCTZHIP_E_ARG, "null stream buffer");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  // the root's own streams first, OUTSIDE the group: a failure here must not leave a group open
  if (me == root) {
    uint64_t ob = 0, od = 0, oa = 0;
    for (int r = 0; r < me; r++) { ob += sizes[3 * r]; od += sizes[3 * r + 1]; oa += sizes[3 * r + 2]; }
    const uint64_t n = sizes[3 * me], nb = sizes[3 * me + 1], cn = sizes[3 * me + 2];
    HIPCHK(c, hipMemcpyAsync((char*)d_bin_all + ob, d_bin, n, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_dc_all + od, d_dc, nb * 4, hipMemcpyDeviceToDevice, s));
    if (cn) HIPCHK(c, hipMemcpyAsync(d_ac_all + oa, d_ac, cn * 4, hipMemcpyDeviceToDevice, s));
  }
  // Every exit between GroupStart and GroupEnd closes the group first: a rank that returned with its group open would
  // never issue its operations while its peers wait in theirs.
  RCCLCHK(c, g_rccl.GroupStart());
  int bad = 0;
  const char* what = "";
#define IN_GROUP(call) do { if (!bad) { bad = (call); if (bad) what = #call; } } while (0)
  if (me == root) {
    uint64_t ob = 0, od = 0, oa = 0;
    for (int r = 0; r < W; r++) {
      const uint64_t n = sizes[3 * r], nb = sizes[3 * r + 1], cn = sizes[3 * r + 2];
      if (r != me) {
        IN_GROUP(g_rccl.Recv((char*)d_bin_all + ob, n, NCCL_UINT8, r, c->comm, s));
        IN_GROUP(g_rccl.Recv(d_dc_all + od, nb, NCCL_FLOAT32, r, c->comm, s));
        if (cn) IN_GROUP(g_rccl.Recv(d_ac_all + oa, cn, NCCL_FLOAT32, r, c->comm, s));
      }
      ob += n; od += nb; oa += cn;
    }
  } else {
    const uint64_t n = sizes[3 * me], nb = sizes[3 * me + 1], cn = sizes[3 * me + 2];
    IN_GROUP(g_rccl.Send(d_bin, n, NCCL_UINT8, root, c->comm, s));
    IN_GROUP(g_rccl.Send(d_dc, nb, NCCL_FLOAT32, root, c->comm, s));
    if (cn) IN_GROUP(g_rccl.Send(d_ac, cn, NCCL_FLOAT32, root, c->comm, s));
  }
#undef IN_GROUP
  const int end = g_rccl.GroupEnd();                  // (always: also after a failed call inside the group)
  if (bad) return fail(c, DCTZHIP_E_HIP, "%s failed: %s", what, g_rccl.GetErrorString(bad));
  if (end) return fail(c, DCTZHIP_E_HIP, "ncclGroupEnd failed: %s", g_rccl.GetErrorString(end));
  HIPCHK(c, hipStreamSynchronize(s));
  return DCTZHIP_OK;
}

