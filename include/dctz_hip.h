/*
 * dctz_hip.h -- C ABI of the MI355X (gfx950) hot path of DCTZ.
 *
 * This is the seam a DCTZ maintainer binds to: it sits INSIDE the reference's
 * dctz_compress() / dctz_decompress() (dctz.h:126-127) and replaces exactly the
 * serial CPU stages between "input in memory" and "three byte streams ready for
 * zlib" (and the mirror image on the way back).  Plain C types only; device
 * buffers are passed as void* device pointers; the library never frees or
 * reallocates caller memory.  Every entry point returns 0 on success or a
 * negative DCTZHIP_E_* code; dctzhip_last_error() gives the text.  There is NO
 * CPU fallback: without a usable HIP device every call fails.
 *
 * Each function names the reference code it replaces (file:line under the
 * upstream tree).
 */
#ifndef DCTZ_HIP_H
#define DCTZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTZHIP_BLK 64            /* dctz.h:28  BLK_SZ */
#define DCTZHIP_NBINS 255         /* dctz.h:65-66 (t_bin_id = unsigned char) */

enum { DCTZHIP_F32 = 0, DCTZHIP_F64 = 1 };   /* values of t_datatype, dctz.h:44-47 */
enum { DCTZHIP_EC = 0, DCTZHIP_QT = 1 };     /* -DUSE_QTABLE off/on, Makefile:12-17 */

enum {
  DCTZHIP_OK = 0,
  DCTZHIP_E_ARG = -1,        /* bad argument (null, misaligned, n == 0, n > INT_MAX) */
  DCTZHIP_E_BOUND = -2,      /* error_bound < 1e-6: dctz-comp-lib.c:135-138 */
  DCTZHIP_E_HIP = -3,        /* a HIP runtime call failed (no device, OOM, ...) */
  DCTZHIP_E_INTERNAL = -4,   /* the library caught itself out: a launch plan that does not fit its scratch tables, a
                                hand-off that never arrived (10 s), an error flag set by a kernel */
  DCTZHIP_E_SPACE = -5       /* dctzhip_fixup_build: the list has more entries than the caller's capacity (*count says how many) */
};

typedef struct dctzhip_ctx dctzhip_ctx;

/* What the compress stage hands back to the host besides the three streams.
 * For DCTZHIP_F32 the stats are float values widened exactly to double. */
typedef struct {
  double sf;                 /* scaling factor, util.c:29/43 (host libm, same expr) */
  double mean;               /* sum/N, util.c:28/41 -- DEVICE summation order       */
  double max_abs, min_abs;   /* util.c:18-25 */
  uint32_t cnt;              /* tot_AC_exact_count, dctz-comp-lib.c:323,497,537     */
  uint32_t nblk;             /* CEIL(N, 64), dctz-comp-lib.c:227                    */
  double qtable[64];         /* QT: clamped table as appended to the stream
                                (dctz-comp-lib.c:450-461, 815-820); slot 0 = DC of
                                the last block (:355-360).  EC: zeros.             */
  double qtable_raw[64];     /* QT: table before clamping (= ./qtable.bin, :443-448) */
  uint32_t flags;            /* DCTZHIP_INFO_*: how the statistics were obtained (below) */
  uint32_t reserved;
} dctzhip_cinfo;

/* calc_data_stat (util.c:12-44) needs the whole array before the first division
 * (dctz-comp-lib.c:193-216), i.e. a second read of the input.  Only the decade of
 * max|x| enters sf (util.c:29), so for large inputs the library guesses sf from a
 * sample, lets the compress kernel compute the TRUE max / min / sum while it
 * streams the data anyway, and checks the guess afterwards.  The outputs never
 * depend on the guess: a wrong one is detected and the kernels run again with
 * the true statistics. */
#define DCTZHIP_INFO_STATS_FUSED 1u   /* guess verified: the separate statistics pass was saved */
#define DCTZHIP_INFO_RESPUN 2u        /* guess wrong: compress kernels were run a second time    */
#define DCTZHIP_INFO_SPLIT 8u         /* the compress kernel was k_compress_eo (a block over two lanes: dctzhip_set_split)          */
#define DCTZHIP_INFO_SINGLE_PASS 16u  /* ... and AC_exact was placed by that kernel itself (look-back over the tiles' counts)       */
#define DCTZHIP_INFO_LB_FALLBACK 32u  /* ... whose look-back gave up: the pass was run again through the workgroup-local lists      */
#define DCTZHIP_INFO_ONE_LAUNCH 4u    /* the whole call was one kernel (arrays whose tiles are all resident at once)         */

/* Per-kernel device time of the last compress / decompress call, milliseconds,
 * measured with HIP events on the context's stream (only when profiling is on). */
typedef struct {
  float stats_ms;            /* calc_data_stat kernels          */
  float main_ms;             /* fused block-DCT + binning (or de-quantise + IDCT) */
  float tail_ms;             /* remainder block + QT normalise   */
  float total_ms;            /* first kernel start -> last kernel end */
} dctzhip_timings;

/* ---- context ------------------------------------------------------------- */
/* device < 0: use the current HIP device.  The context owns a stream, constant
 * tables and a scratch arena that grows on demand (dctzhip_reserve pre-sizes it
 * so that later calls do no allocation).  One context per GPU per thread of
 * control; a context is not re-entrant (neither is the reference: file-static
 * FFTW plan, dct.c:18-22). */
int dctzhip_device_count(void);                            /* GPUs visible to this process (0 if none) */
int dctzhip_ctx_create(dctzhip_ctx **out, int device);
void dctzhip_ctx_destroy(dctzhip_ctx *ctx);
const char *dctzhip_last_error(const dctzhip_ctx *ctx);   /* ctx may be NULL: last create error */
int dctzhip_reserve(dctzhip_ctx *ctx, size_t n, int dtype, int mode);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * context's own.  NULL is the legacy default stream, as everywhere in HIP (what a
 * caller that never created a stream runs on -- ordered against its other work);
 * dctzhip_use_own_stream goes back to the context's private non-blocking stream.
 * Moving a context between streams: its scratch arena, control blocks and tables are
 * ordered by the stream it ran on, and a call's last kernels may still be running there
 * when the call returns.  Before binding another stream the caller either completes the
 * old one (hipStreamSynchronize) or orders the new one behind it (an event recorded on
 * the old stream that the new one waits for).  The library itself records nothing on a
 * stream it is told to leave -- the caller may have destroyed it already -- and queues no
 * wait on the new one; both calls only drop the decode memo.  (dctz_amd.Context, which
 * follows torch's current stream on the caller's behalf, does this ordering itself.) */
int dctzhip_set_stream(dctzhip_ctx *ctx, void *hip_stream);
int dctzhip_use_own_stream(dctzhip_ctx *ctx);
void *dctzhip_get_stream(dctzhip_ctx *ctx);
int dctzhip_set_profiling(dctzhip_ctx *ctx, int on);
/* Speculative fused statistics (see DCTZHIP_INFO_*): on != 0 enables it for inputs of
 * at least min_elements (0 keeps the current threshold, default 2^22); on == 0 always
 * runs the separate statistics pass first.  Default: on (env DCTZHIP_SPECULATE=0 turns
 * it off).  d_scaled holds x / sf for the verified sf when the call returns: k_compress
 * writes it while it runs (a pass with a wrong guess is run again and writes it again); a
 * call whose d_scaled aliases d_in does not speculate (the input would not survive a wrong
 * guess) and takes the full statistics pass first.  DCTZHIP_FUSE_SCALED=0: a pass of its
 * own behind the kernels, as before round 3. */
int dctzhip_set_speculation(dctzhip_ctx *ctx, int on, size_t min_elements);
/* The guess without a sample.  A speculative call (above) whose input -- the same d_in, n and dtype -- was compressed by
 * the last two or more speculative calls with one and the same verified scaling factor guesses from the TRUE statistics of
 * the last of them instead of sampling: the two statistics launches in front of the compress kernel fall away (a field of a
 * time-stepping code, a snapshot slot).  The guess is verified exactly as a sampled one is and the streams never depend on
 * it; a wrong one costs what a wrong sample costs (one re-run, then 8 calls on the full statistics pass) and doubles the
 * number of verified sampled calls the input needs before it is trusted again (2, 4, ... at most 64).  The context
 * remembers 8 inputs, the least recently used one replaced.  info->flags does not tell the two kinds of guess apart
 * (DCTZHIP_INFO_STATS_FUSED / _RESPUN); dctzhip_debug_counter 18 / 19 do.  on == 0: every speculative call samples; either
 * value clears what is remembered, and so does dctzhip_set_speculation(ctx, 0, ..).  An input the library owns (the filled
 * copy of dctzhip_compress_masked without d_filled) is never remembered: such calls sample.  Turn it off for a caller that rotates
 * unrelated fields through one buffer.  Default: on (env DCTZHIP_SPEC_MEMORY=0 turns it off). */
int dctzhip_set_spec_memory(dctzhip_ctx *ctx, int on);
int dctzhip_last_timings(dctzhip_ctx *ctx, dctzhip_timings *t);
/* One launch per call.  An array whose tiles are all resident on the chip at once (up to about 8 M fp32 / 4 M fp64 elements:
 * 2048 / 1024 tiles of 64 blocks) is compressed -- and decompressed -- by ONE kernel: calc_data_stat, scaling, transform,
 * binning and the ordered placement of AC_exact (decode: flag counts, their prefix, reconstruction) exchange what the chain
 * of kernels hands over at kernel boundaries through 8-byte tagged words in device memory instead.  The outputs are bit for
 * bit the chain's (DCTZHIP_INFO_ONE_LAUNCH in info->flags tells which ran); a launch that finds its workgroups not all
 * resident (another process on the GPU) gives up after 20 ms and the call is run through the chain.  Default: on (env
 * DCTZHIP_ONE=0 turns it off); on == 0 always takes the chain of kernels. */
int dctzhip_set_one_launch(dctzhip_ctx *ctx, int on);
/* A block over two lanes.  on != 0: the compress kernel of the chain (arrays beyond the one-launch size) for flat fp64
 * blocks is k_compress_eo -- workgroups of two wavefronts that share a tile's blocks, one computing the even-numbered
 * coefficients of every block, the other the odd-numbered ones (half the registers per lane, three waves per SIMD instead
 * of two) -- with the tile's exact coefficients put into the reference's order inside the kernel.  Outputs are bit for bit
 * those of k_compress.  Calls that ask for the scaled copy, fp32 and multi-dimensional blocks keep k_compress.
 * on == 3, EC mode (experimental: measured slower than the lists): the kernel also writes every exact coefficient at its
 * final place in AC_exact[] -- tiles are handed out in order by ticket counters, each posts its count and looks back over
 * the counts in front of it for the running tot_AC_exact_count (dctz-comp-lib.c:478-544) -- so the call has no
 * workgroup-local lists and no k_compact_ac pass (DCTZHIP_INFO_SINGLE_PASS); a look-back that sees no progress for 20 ms
 * gives up and the pass is run again through the lists (DCTZHIP_INFO_LB_FALLBACK).  Env DCTZHIP_EO=0/1 and
 * DCTZHIP_EO_DIRECT=0/1 set the defaults (off, off). */
int dctzhip_set_split(dctzhip_ctx *ctx, int on);
/* The decode memo.  A dctzhip_compress call on the chain of kernels (flat blocks, k_compress + k_compact_ac) leaves in the
 * context, per tile of 64 blocks, the count of its exact coefficients and their first place in AC_exact[].  A
 * dctzhip_decompress call on the same context and stream whose d_bin, d_dc, d_ac, n, dtype, mode are that call's and whose
 * ac_count is its total (fp64 EC, n a multiple of 64, mailbox hand-off on) starts from those tables instead of counting the
 * flags of bin_index in a pass of its own.  The tables are checked, not trusted: the decoder compares every tile's count
 * with the flags it reads; if the buffers were rewritten in between so that any count differs, the same call decodes
 * again the classic way and returns what that gives (its refusal of an under-run included).  With all counts equal the
 * reconstruction is the classic decoder's bit for bit.  Any later compress call of the context (single, part, batch, N-D)
 * and dctzhip_set_stream drop the memo.  Default: on (env DCTZHIP_DEC_MEMO=0 turns it off); counters 16 / 17 below. */
int dctzhip_set_decode_memo(dctzhip_ctx *ctx, int on);
/* (tests and tools)  Counters of the context -- which: 0 one-launch calls, 1 one-launch launches that gave up (run again
 * through the chain), 2 calls left on the chain after such a launch, 3 calls through k_compress_eo, 4 of them with
 * single-pass placement, 5 look-backs that gave up, 6 / 7 verified / wrong guesses of the scaling factor, 8 / 9 speculative
 * items of batches / those whose guess was refused, 10 step-downs of dctzhip_compress_psnr / _psnr_nd, 11 / 12 workgroups and
 * candidate tiles of the last dctzhip_decompress_box / _box_nd / _coarse_box_nd call, whichever ran last (12 > 11: its
 * grid-stride loop ran; a _coarse_box_nd call with factor == block edge reads no tiles: 12 is 0), 13 / 14 / 15 items
 * in the list of the last dctzhip_decompress_boxes, _boxes_nd or _coarse_boxes_nd call (whichever of them ran last),
 * workgroups of its decode launch and the list's bound, 16 / 17
 * dctzhip_decompress calls launched on the decode memo / of them found stale and decoded again, 18 / 19 guesses of the
 * scaling factor taken from the remembered statistics of the same input that verified / that did not, 20 the division
 * and binning variant of the last verified pass of the last dctzhip_compress / _compress_nd call: fast_sf | fast_bw << 8
 * (fast_sf 0 plain x / sf, 1 FastDiv with a per-element window test, 2 without; fast_bw bit 0 the bin width is in
 * FastDiv's divisor window, bit 1 the kernels drop the range test of the binning: 3, 1 or 0; where the device chose sf,
 * fast_sf is what it reported) -- and knobs that
 * make a rare path run on purpose -- key 0: workgroup 0 of the one-launch kernels withholds its granule (the launch gives
 * up after 20 ms, the call is run through the chain), 1: one look-back of k_compress_eo gives up, 2: sets counter 2,
 * 3: every predicted SSE of dctzhip_rd_probe / _rd_probe_nd is divided by value (value <= 1: off), 4: sets the tag of the
 * last one-launch kernel to value's 32 bits (-3: 2^32 - 3), so that the next calls meet the wrap of the tag, on which the
 * board of granules is cleared. */
int dctzhip_debug_counter(dctzhip_ctx *ctx, int which, unsigned long long *value);
int dctzhip_debug_knob(dctzhip_ctx *ctx, int key, int value);
/* (tools) the name rocprofv3 lists the big kernel of the last call under, every template argument: which = 0 compress,
 * 1 decompress (the random-access calls included), 2 / 3 batch compress of the fp64 / fp32 arrays, 4 / 5 batch decompress ("" if none ran yet) */
int dctzhip_debug_last_kernel(dctzhip_ctx *ctx, int which, char *buf, size_t cap);
/* on != 0: every compress / decompress call ends with a synchronisation of the context's stream, i.e. its outputs are
 * complete for ANY observer when it returns (default off: complete in stream order, see the two calls below; env
 * DCTZHIP_BLOCKING=1 does the same).  For callers that read the buffers from another stream or from the host without
 * going through the context's stream. */
int dctzhip_set_blocking(dctzhip_ctx *ctx, int on);

/* ---- device memory helpers (so plain-C hosts need no HIP headers) --------- */
int dctzhip_malloc(dctzhip_ctx *ctx, void **dptr, size_t bytes);
int dctzhip_free(dctzhip_ctx *ctx, void *dptr);
int dctzhip_memcpy_h2d(dctzhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int dctzhip_memcpy_d2h(dctzhip_ctx *ctx, void *dst, const void *src, size_t bytes);
int dctzhip_sync(dctzhip_ctx *ctx);
/* A D2H copy on a stream BESIDE the context's, for a second host thread (the pipelined dctz_compress brings finished pieces
 * back while the calling thread queues the next kernels): the caller has synchronised with whatever produced d_src, and
 * makes such copies from one thread at a time. */
int dctzhip_memcpy_d2h_side(dctzhip_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* A D2H copy into pageable host memory that FOLLOWS its producer (dctz_decompress rebuilds a large array group by group
 * and brings finished groups back while the next ones are built): begin() starts the copy of bytes [0, bytes) of d_src to
 * dst through pinned slots, piece by piece, each piece as soon as advance() has announced it -- "bytes [0, upto) are
 * complete in the order of the context's stream" (an event behind the kernels queued so far; no host synchronisation) --,
 * end() waits for the last piece (abandon != 0: stops after the pieces under way).  One pipe at a time per process. */
/* capacities of the two pipes below: dctzhip_d2h_pipe_advance may be called this many times per pipe, a dctzhip_h2d_pipe_begin
 * takes at most this many groups (a caller with more takes its unpipelined path instead) */
#define DCTZHIP_D2H_PIPE_MAX_MARKS 256
#define DCTZHIP_H2D_PIPE_MAX_GROUPS 4096
int dctzhip_d2h_pipe_begin(dctzhip_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int dctzhip_d2h_pipe_advance(dctzhip_ctx *ctx, size_t upto);
int dctzhip_d2h_pipe_end(dctzhip_ctx *ctx, int abandon);
/* An H2D copy from pageable host memory whose CONSUMER follows it (dctz_compress of a large array starts the kernels of a
 * group of elements as soon as that group is on the device): begin() starts the copy of src[0, bytes) to d_dst in groups
 * of group_bytes, in order, on a stream of its own; wait(upto) makes the context's stream wait -- on the GPU -- for the
 * group that holds byte upto - 1 (the host waits only until that group's copy has been issued); landed(upto) blocks the
 * host until bytes [0, upto) are on the device, i.e. until the source range is no longer read; end() joins (abandon != 0:
 * no further group is issued).  One pipe at a time per process. */
int dctzhip_h2d_pipe_begin(dctzhip_ctx *ctx, void *d_dst, const void *src, size_t bytes, size_t group_bytes);
int dctzhip_h2d_pipe_wait(dctzhip_ctx *ctx, size_t upto);
int dctzhip_h2d_pipe_landed(dctzhip_ctx *ctx, size_t upto);
int dctzhip_h2d_pipe_end(dctzhip_ctx *ctx, int abandon);
/* Page-lock a caller-owned host buffer for the copies above (hipHostRegister): pageable copies run at about 24 GB/s,
 * pinned ones at PCIe speed.  Pinning itself costs about as much as one pageable copy of the buffer, so it pays for
 * buffers that are reused across calls; the buffer must be unregistered before it is freed. */
int dctzhip_host_register(dctzhip_ctx *ctx, void *ptr, size_t bytes);
int dctzhip_host_unregister(dctzhip_ctx *ctx, void *ptr);

/* ---- compress stage ------------------------------------------------------ */
/* Replaces dctz-comp-lib.c:186-217 (calc_data_stat + scale, util.c:12-44),
 * :271-281 (bin ranges), :318-416 (dct_init + per-block dct_fftw + DC + pass-1
 * binning), :435-476 (QT table) and :478-544 (pass-2 exception compaction).
 *   d_in        n elements (float|double), device, 16-byte aligned; not modified
 *   d_bin_index n bytes out (bin ids; 255 = DC slot / stored exactly)
 *   d_dc        nblk floats out (USE_TRUNCATE)
 *   d_ac_exact  capacity n floats out; info->cnt of them are valid, block-major,
 *               j ascending -- byte-identical to the reference's AC_exact[]
 *   d_scaled    optional: receives x/sf (the reference's in-place scaling of the
 *               caller's buffer, :193-216); may be NULL, may alias d_in (then the
 *               call runs on verified statistics: see dctzhip_set_speculation).
 *               Like every output it is complete in STREAM order, not at return
 *               (single arrays and batches alike), unless dctzhip_set_blocking is on
 *   d_coef      optional debug tap: the DCT coefficients a_x after pass 1
 *               (= dct_result.bin under -DDCT_FILE_DEBUG, :422-428); may be NULL
 * On return *info is filled (the host has waited for it); the last kernels of the
 * call may still be running: the output buffers are complete in STREAM order --
 * for any later call or copy on the context's stream, or after dctzhip_sync().
 * Buffers of one call: no output (d_bin_index n bytes, d_dc nblk floats, d_ac_exact
 * its capacity of n floats, d_scaled unless it is d_in, d_coef) may overlap d_in or
 * another output; d_scaled either is d_in exactly or lies clear of it.  Anything else
 * returns DCTZHIP_E_ARG before a launch. */
int dctzhip_compress(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype,
                     double error_bound, int mode, void *d_bin_index, float *d_dc,
                     float *d_ac_exact, void *d_scaled, void *d_coef,
                     dctzhip_cinfo *info);

/* A PART of an array whose statistics the caller already has (EC mode).  The streams of elements [lo, lo + n) of an array
 * are the same whether the array is compressed in one call or part by part -- blocks are independent
 * (dctz-comp-lib.c:323-416), AC_exact is block-major (:478-544) -- provided every part is scaled by the ARRAY's scaling
 * factor (util.c:29), the one thing that couples them: max_abs / min_abs are max|x| and min|x| of the WHOLE array
 * (calc_data_stat, util.c:18-25).  Parts start on block boundaries (lo % 64 == 0); only the array's last part may end in
 * a short block.  d_bin / d_dc: the part's own positions (bin_index + lo, DC + lo / 64); d_ac: where the part's exact
 * coefficients go -- AC_exact + the counts of the parts in front; *cnt: the part's count; part_stats (or NULL): max|x|,
 * min|x| of the part and the sum of its elements from the SECOND on (util.c:22 starts at i = 1: the caller adds a part's
 * first element unless the part is the array's first); *sf (or NULL): the scaling factor used.  A part whose own extremes
 * lie outside [min_abs, max_abs] is refused (DCTZHIP_E_ARG: the statistics are not this array's).  NaN elements are passed
 * over by the statistics wherever they stand: the pair of an array that holds nothing else is
 * max_abs = 0, min_abs = the largest finite value of the element type, as dctzhip_stats reports it, and is accepted. */
int dctzhip_compress_part(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, double error_bound, double max_abs,
                          double min_abs, void *d_bin, float *d_dc, float *d_ac, uint32_t *cnt, double *part_stats, double *sf);

/* calc_data_stat alone (util.c:12-44): fills sf, mean (device order), max_abs,
 * min_abs and nblk of *info. */
int dctzhip_stats(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, dctzhip_cinfo *info);

/* The header's `mean` in the reference's SERIAL summation order (util.c:18-28:
 * sum of x[1..N-1] in the data type, then / N) -- bit-identical to the
 * reference, which a parallel reduction cannot be.  begin() enqueues a
 * single-wavefront kernel on a side stream and returns at once; end() waits
 * for it.  The kernel is ordered behind everything that is queued on the context's
 * stream when begin() is called (an event there that the side stream waits for), so
 * d_in may still be in the making on that stream; nothing later on the context's stream
 * waits for the side stream, so d_in must stay unmodified until end() has returned.
 * (~0.5 s per GiB of fp64: meant
 * to run underneath the host zlib tail, which is 20x longer.) */
int dctzhip_serial_mean_begin(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype);
int dctzhip_serial_mean_end(dctzhip_ctx *ctx, double *mean);

/* x[i] /= sf in place on the device (dctz-comp-lib.c:193-216), no-op if sf == 1.
 * Synchronous. */
int dctzhip_scale_inplace(dctzhip_ctx *ctx, void *d_x, size_t n, int dtype, double sf);

/* ---- decompress stage ---------------------------------------------------- */
/* Replaces dctz-decomp-lib.c:358-361 (gen_bins, binning.c:12-50), :372-386,
 * :389-483 (de-quantise + ifft_idct per block) and :494-511 (de-scale).
 *   ac_count     number of valid floats in d_ac_exact (header.tot_AC_exact_count);
 *                a bin_index that flags more than that fails with DCTZHIP_E_ARG
 *   qtable_host  QT: the 64 table values in the data type, HOST memory (as read
 *                from the stream tail, dctz-decomp-lib.c:193-199); EC: NULL
 *   sf           header scaling factor (scaling_factor.d, or .f widened)
 *   d_out        n elements out; must not overlap d_bin_index (n bytes), d_dc (nblk
 *                floats) or the ac_count floats of d_ac_exact (else DCTZHIP_E_ARG
 *                before a launch)
 *   alignment    d_bin_index and d_out 16-byte aligned; DC, AC_exact: 4-byte aligned (else
 *                DCTZHIP_E_ARG before a launch) -- dctzhip_decompress_nd and the items of
 *                dctzhip_decompress_batch alike
 * Returns once the stream is known to be consistent with ac_count (the only thing the
 * host has to learn); the reconstruction itself is complete in STREAM order -- for
 * any later call or copy on the context's stream, or after dctzhip_sync(). */
int dctzhip_decompress(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc,
                       const float *d_ac_exact, uint32_t ac_count,
                       const void *qtable_host, size_t n, int dtype,
                       double error_bound, double sf, int mode, void *d_out);

/* ---- random access on decode ------------------------------------------------ */
/* The blocks of a stream are independent but for the running position `pos` in AC_exact (dctz-decomp-lib.c:370,
 * :402-412): the number of "stored exactly" flags in front of a block.  The exception index holds it every
 * DCTZHIP_INDEX_STRIDE elements.  With m = ceil(n / 4096), for 0 <= i <= m
 *   idx[i] = number of bin ids equal to 255 at an in-block position j, 1 <= j < block length, in elements
 *            [0, min(n, 4096 i))
 * (the DC slot does not count, nor anything past the short last block): idx[i] is the reference's pos at block 64 i and
 * idx[m] is tot_AC_exact_count.  Built from bin_index alone, so it serves any streams -- this library's or those
 * inflated from a reference container -- and EC and QT alike.  Nothing is written into containers.
 *   dctzhip_ac_index_len  entries of the index: ceil(n / 4096) + 1
 *   dctzhip_ac_index      d_bin_index (n bytes, 16-byte aligned) -> d_index (dctzhip_ac_index_len(n) words, 4-byte
 *                         aligned, not overlapping bin_index); *total (or NULL) receives idx[m].  1 <= n <= INT_MAX.
 *                         Host-synchronous, like dctzhip_stats. */
#define DCTZHIP_INDEX_STRIDE 4096   /* elements per index entry (64 blocks) */
size_t dctzhip_ac_index_len(size_t n);
int dctzhip_ac_index(dctzhip_ctx *ctx, const void *d_bin_index, size_t n, uint32_t *d_index, uint32_t *total);
/* Elements [lo, hi) of the array, 0 <= lo < hi <= n, any alignment.  The streams and d_index describe the WHOLE array and
 * are passed as pointers to its start, exactly as for dctzhip_decompress (ac_count, qtable_host, n, dtype, error_bound,
 * sf and mode mean what they mean there).
 *   d_out       receives hi - lo elements: d_out[k] is, bit for bit, element lo + k of what dctzhip_decompress writes for
 *               the same arguments (EC and QT, fp32 and fp64, the short last block included)
 *   locality    with t0 = lo / 4096 and t1 = ceil(hi / 4096) the call reads only the bin ids and DC values of tiles
 *               [t0, t1), the index entries idx[t0 .. t1] and AC_exact[idx[t0], idx[t1]); it writes nothing outside
 *               d_out[0, hi - lo).  Its cost follows the range, not n.
 *   refusals    before any launch, DCTZHIP_E_ARG for a range outside [0, n), a null or misaligned pointer (bin_index and
 *               d_out 16-byte aligned, DC, AC_exact and the index 4-byte aligned), and a d_out that overlaps what the call
 *               reads (bin ids and DC of the range's tiles, their index entries, AC_exact[0, ac_count)).  On the device:
 *               the flags of every tile t of the range must number idx[t + 1] - idx[t], and idx[t1] <= ac_count; if not,
 *               DCTZHIP_E_ARG as for dctzhip_decompress's under-run, the output is undefined and the context stays usable.
 * Returns once that check is known; the output is complete in stream order on the context's stream (and the call has
 * synchronised the stream). */
int dctzhip_decompress_range(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                             uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                             double error_bound, double sf, int mode, size_t lo, size_t hi, void *d_out);
/* A rectangular box of the array seen as an ndim-dimensional array in C order (last dimension fastest), 1 <= ndim <=
 * DCTZHIP_BOX_MAXDIM, prod dims == n: the elements lo[i] <= c[i] < hi[i] in every dimension.  The streams, d_index,
 * ac_count, qtable_host, n, dtype, error_bound, sf and mode are dctzhip_decompress_range's: they describe the WHOLE array,
 * compressed in the ordinary flat 64-element blocks (dctzhip_compress); streams in the tiles of dctzhip_compress_nd have
 * dctzhip_decompress_box_nd.
 * Fortran order: reverse dims, lo and hi.
 *   d_out       receives prod (hi[i] - lo[i]) elements, dense, in C order; each is, bit for bit, the element that
 *               dctzhip_decompress writes at the same coordinates (EC and QT, fp32 and fp64, the short last block
 *               included).  ndim == 1 gives the bytes of dctzhip_decompress_range(lo[0], hi[0]).
 *   locality    a tile (4096 consecutive elements) is HIT if at least one of its elements lies in the box.  The call reads
 *               the bin ids and DC values of hit tiles only, their index entries idx[t] and idx[t + 1] only, and
 *               AC_exact[idx[t], idx[t + 1]) of hit tiles only; it writes nothing outside d_out[0, prod ext).  A hit tile
 *               is decoded once however many rows of the box cross it: the cost follows the number of hit tiles, not n and
 *               not the number of rows.
 *   refusals    before any launch, DCTZHIP_E_ARG for ndim outside 1 .. 4, a null dims, lo or hi, a zero extent, prod dims
 *               != n, lo[i] >= hi[i] or hi[i] > dims[i], the pointer and alignment rules of dctzhip_decompress_range, and
 *               a d_out that overlaps what dctzhip_decompress_range may read for [first box element, last box element +
 *               1).  On the device, for hit tiles only: the flags of tile t must number idx[t + 1] - idx[t], and idx[t +
 *               1] <= ac_count; if not the tile reads no AC_exact and the call returns DCTZHIP_E_ARG, the output is
 *               undefined and the context stays usable.
 * Returns once that check is known, as dctzhip_decompress_range does. */
#define DCTZHIP_BOX_MAXDIM 4
int dctzhip_decompress_box(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                           uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                           double error_bound, double sf, int mode, int ndim, const size_t *dims, const size_t *lo,
                           const size_t *hi, void *d_out);
/* k boxes of the SAME array in one call: one box table handed over in one transfer, one work list of (box, hit tile) pairs
 * built on the device, one persistent decode launch whose workgroups take list items -- none of them ever meets a tile
 * that is not hit -- and one synchronisation.  Everything but the last two arguments is dctzhip_decompress_box's; boxes is
 * a HOST array of k items, entries of lo / hi at positions >= ndim are ignored.
 *   boxes[i].d_out  receives exactly the bytes dctzhip_decompress_box writes for box i with the same remaining arguments
 *               (EC and QT, fp32 and fp64, the short last block included)
 *   overlap     boxes may overlap, nest or repeat.  A tile hit by two boxes is decoded once per box that hits it:
 *               de-duplication is not part of this call.
 *   locality    that of dctzhip_decompress_box over the union of the boxes' hit tiles: the call reads the bin ids, DC
 *               values, idx[t], idx[t + 1] and AC_exact[idx[t], idx[t + 1]) of tiles hit by at least one box and nothing
 *               else of the streams; it writes nothing outside the k outputs.
 *   refusals    before anything is launched or written, all or nothing, DCTZHIP_E_ARG: k < 1, k > DCTZHIP_BOXES_MAX, a null
 *               boxes; for any box whatever dctzhip_decompress_box refuses (the message names the box's index); an output
 *               that overlaps another output or what any box of the call may read; boxes that may hit more than 2^24 tiles
 *               in all (the bound of the work list: per box the smaller of its candidate tiles and the tiles its rows can
 *               touch).  On the device, for hit tiles only, dctzhip_decompress_box's index check: a failing tile reads no
 *               AC_exact, the call returns DCTZHIP_E_ARG, the outputs are undefined and the context stays usable.
 * Returns once that check is known, having synchronised the context's stream once, as dctzhip_decompress_box does.
 *   cost        the list builder runs one thread per (box, candidate tile), candidates being the tiles from a box's first
 *               to its last element: cheap next to a decode (a rank computation each), but it follows the candidates, not the
 *               hits.  Thousands of thin boxes that each span a large array (up to 2^31 pairs in all) pay for that span;
 *               only the hits are bounded (2^24).
 * dctzhip_debug_counter 13 / 14 / 15: items of the last call's list, workgroups of its decode launch, the list's bound. */
#define DCTZHIP_BOXES_MAX 4096
typedef struct { size_t lo[DCTZHIP_BOX_MAXDIM], hi[DCTZHIP_BOX_MAXDIM]; void *d_out; } dctzhip_box_item;
int dctzhip_decompress_boxes(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                             uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                             double error_bound, double sf, int mode, int ndim, const size_t *dims,
                             int k, const dctzhip_box_item *boxes /* host */);

/* ---- batches of arrays ------------------------------------------------------ */
/* The reference's own workloads are LISTS of small arrays, one dctz_compress() call and one process each
 * (tests/test-dctz.sh:13-56 over tests/list-msst19.txt:1-6: 12 960 ... 37 024 doubles; tests/list-CESM-ATM-tylor.txt:1-5).
 * On a GPU one such call is four or five launches and a host hand-off around a few microseconds of kernel work.  A batch
 * runs k arrays -- own element type, error bound, buffers and results each; nothing in the reference couples two arrays
 * (own calc_data_stat, sf, bin ranges, tot_AC_exact_count, QT table: dctz-comp-lib.c:186 onwards) -- through ONE launch
 * sequence per element type with ONE hand-off.  Every array's outputs (streams, scaled copy, *info) are bit for bit
 * those of its own dctzhip_compress() / dctzhip_decompress() call.  Arrays of 2^24 elements or more are handed to the
 * single-array path inside the call (their kernels dwarf the launch cost, and that path saves the statistics pass).
 * Fields have the meaning of the same-named arguments of dctzhip_compress / dctzhip_decompress.
 *
 * Buffers shared between items of a compress batch:
 *   - every item compresses its d_in as it was when the call was made;
 *   - any number of items may read the same or overlapping input ranges, with any dtype (a bound sweep over one array
 *     reads it once for all of them);
 *   - an item scales in place only with d_scaled == d_in exactly; its buffer ends as that item's x / sf, written after
 *     every read of the call (an input another item reads is divided at the very end of the call);
 *   - DCTZHIP_E_ARG, before anything is launched: two in-place items whose ranges overlap; a d_scaled that is not its
 *     item's d_in and overlaps any input; any output (d_bin_index n bytes, d_dc nblk floats, d_ac_exact its capacity of
 *     n floats, d_scaled) that overlaps another output or any input.
 * Items of a decode batch may share their inputs; d_out must not overlap any item's inputs or another d_out (E_ARG). */
typedef struct {
  const void *d_in;          /* n elements of dtype, device, 16-byte aligned; not modified unless d_scaled is d_in */
  size_t n;
  int dtype;                 /* DCTZHIP_F32 | DCTZHIP_F64, per array */
  double error_bound;        /* per array */
  void *d_bin_index;         /* n bytes out */
  float *d_dc;               /* ceil(n / 64) floats out */
  float *d_ac_exact;         /* capacity n floats out */
  void *d_scaled;            /* optional: x / sf (dctz-comp-lib.c:193-216); may be NULL, may be d_in exactly */
} dctzhip_batch_citem;
typedef struct {
  const void *d_bin_index;   /* 16-byte aligned, like d_out */
  const float *d_dc;         /* DC, AC_exact: 4-byte aligned */
  const float *d_ac_exact;
  uint32_t ac_count;         /* header.tot_AC_exact_count of this array */
  const void *qtable_host;   /* QT: 64 values in the data type, host memory; EC: NULL */
  size_t n;
  int dtype;
  double error_bound;
  double sf;                 /* header scaling factor of this array */
  void *d_out;               /* n elements out */
} dctzhip_batch_ditem;
/* infos: k entries (may be NULL).  On return every infos[i] is filled; outputs are complete in STREAM order. */
int dctzhip_compress_batch(dctzhip_ctx *ctx, int k, const dctzhip_batch_citem *items, int mode, dctzhip_cinfo *infos);
/* status: k entries (may be NULL): DCTZHIP_OK, or DCTZHIP_E_ARG for an array whose bin_index flags more exact coefficients
 * than its ac_count provides (the call then returns DCTZHIP_E_ARG; the other arrays are reconstructed all the same). */
int dctzhip_decompress_batch(dctzhip_ctx *ctx, int k, const dctzhip_batch_ditem *items, int mode, int *status);
/* Device time of the last batch call per element-type sequence, t[DCTZHIP_F32] and t[DCTZHIP_F64] (profiling on):
 * stats_ms = statistics + scaling factors (decode: flag counts), main_ms = k_compress_batch / k_decompress_batch,
 * tail_ms = remainder blocks + QT maxima + list placement + scaled copies. */
int dctzhip_last_batch_timings(dctzhip_ctx *ctx, dctzhip_timings t[2]);

/* ---- multi-dimensional blocks (optional mode) ------------------------------ */
/* SURVEY section 8 f4.  NOT a path of the reference's library, which treats every array as flat
 * (dctz-test.c:77-91); the hint is its stand-alone experiment dct-fftw-test.c:74-97 (FFTW_REDFT10 /
 * FFTW_REDFT01 along every axis of a 2-D / 3-D array).  Here the 64 values of a block are an 8 x 8 tile
 * (ndims = 2) or a 4 x 4 x 4 tile (ndims = 3) of the array -- dims[] row-major, last axis fastest, edge tiles
 * padded by repeating the last sample -- transformed with the separable orthonormal DCT-II / DCT-III; tiles
 * are numbered row-major over the tile grid and coefficients row-major inside a tile (position 0 = DC).
 * Everything after the transform is the 1-D pipeline (DC, bins, AC_exact order, QT table per position), so the
 * three streams have the reference's meaning over nblk = prod ceil(dims[i] / edge) blocks:
 *   d_bin_index  nblk * 64 bytes,  d_dc  nblk floats,  d_ac_exact  capacity nblk * 64 floats.
 * Statistics (sf, mean) are those of the original array.  Arrays whose extents are multiples of the tile edge (and
 * below 4 GiB) are read and written in place by the big kernels, at the flat path's speed; ragged ones go through a
 * gather / scatter pass (+2 element sizes of HBM traffic per element and direction).  dctzhip_nd_blocks returns nblk
 * (0 for bad arguments). */
#define DCTZHIP_GEOM_1D 0
#define DCTZHIP_GEOM_2D 1
#define DCTZHIP_GEOM_3D 2
size_t dctzhip_nd_blocks(int ndims, const size_t *dims);
int dctzhip_compress_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype,
                        double error_bound, int mode, void *d_bin_index, float *d_dc,
                        float *d_ac_exact, void *d_scaled, dctzhip_cinfo *info);
int dctzhip_decompress_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc,
                          const float *d_ac_exact, uint32_t ac_count, const void *qtable_host,
                          int ndims, const size_t *dims, int dtype, double error_bound, double sf,
                          int mode, void *d_out);
/* A rectangular box lo[i] <= c[i] < hi[i] of an array compressed by dctzhip_compress_nd(ndims, dims).  The streams,
 * ac_count, qtable_host, ndims, dims, dtype, error_bound, sf and mode are dctzhip_decompress_nd's; they cover n_lin = 64 *
 * dctzhip_nd_blocks(ndims, dims) positions, and d_index is dctzhip_ac_index(d_bin_index, n_lin).
 *   d_out       receives prod (hi[i] - lo[i]) elements, dense, in C order; each is, bit for bit, the element that
 *               dctzhip_decompress_nd writes at the same coordinates (EC and QT, fp32 and fp64, whether the full decode
 *               writes the array in place or through its scatter pass).
 *   locality    a STREAM TILE is 64 consecutive blocks of the stream (4096 positions, one index entry).  The blocks that
 *               intersect the box are, per axis, [lo / e, (hi - 1) / e] (e = 8 | 4): a box of the block grid, which is
 *               numbered row-major.  A stream tile is HIT if it holds at least one of them; candidate tiles run from the
 *               first to the last intersecting block.  The call reads the bin ids and DC values of hit tiles only, their
 *               index entries idx[t] and idx[t + 1] only, and AC_exact[idx[t], idx[t + 1]) of hit tiles only; it writes
 *               nothing outside d_out[0, prod ext).  A hit tile is decoded once.
 *   refusals    before any launch, DCTZHIP_E_ARG for a NULL ctx, whatever dctzhip_decompress_nd refuses for ndims / dims,
 *               a null lo or hi, lo[i] >= hi[i] or hi[i] > dims[i], the pointer and alignment rules of
 *               dctzhip_decompress_box, a QT call without a table, and a d_out that overlaps what the call may read for
 *               the candidate tiles (their bin ids, DC values and index entries, AC_exact[0, ac_count)).  On the device,
 *               for hit tiles only: the flags of tile t must number idx[t + 1] - idx[t], and idx[t + 1] <= ac_count; if
 *               not the tile reads no AC_exact and the call returns DCTZHIP_E_ARG, the output is undefined and the
 *               context stays usable.
 * Returns once that check is known, as dctzhip_decompress_box does (the call has synchronised the stream). */
int dctzhip_decompress_box_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                              uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                              const size_t *dims, int dtype, double error_bound, double sf, int mode,
                              const size_t *lo, const size_t *hi, void *d_out);
/* k boxes of the SAME tiled array in one call: dctzhip_decompress_boxes for the streams of dctzhip_compress_nd.  Everything
 * but the last two arguments is dctzhip_decompress_box_nd's; boxes is a HOST array of 1 <= k <= DCTZHIP_BOXES_MAX items, the
 * first ndims entries of lo / hi are used.  One box table handed over in one transfer, one work list of (box, hit stream
 * tile) pairs built on the device from the boxes of the block grid, one persistent decode launch whose workgroups take list
 * items -- none of them ever meets a candidate tile that is not hit -- and one synchronisation.
 *   boxes[i].d_out  receives exactly the bytes dctzhip_decompress_box_nd writes for box i with the same remaining
 *               arguments (EC and QT, fp32 and fp64, block-aligned and ragged extents)
 *   overlap     boxes may overlap, nest or repeat.  A stream tile hit by m boxes is decoded m times: de-duplication is
 *               not part of this call.
 *   locality    the call reads the bin ids, DC values, idx[t], idx[t + 1] and AC_exact[idx[t], idx[t + 1]) of stream tiles
 *               hit by at least one box and nothing else of the streams; it writes nothing outside the k outputs (padded
 *               positions of edge blocks are never stored).
 *   refusals    before anything is launched or written, all or nothing, DCTZHIP_E_ARG: k < 1, k > DCTZHIP_BOXES_MAX, a null
 *               boxes; whatever dctzhip_decompress_box_nd refuses for ctx, ndims, dims, the streams and the QT table; for
 *               any box what it refuses for lo, hi and d_out (the message names "box i"); an output that overlaps another
 *               output or what any box of the call may read (its candidate tiles' bin ids, DC values and index entries,
 *               AC_exact[0, ac_count)); boxes that may hit more than 2^24 stream tiles in all (the bound of the work list:
 *               per box the smaller of its candidate tiles and the tiles its runs of blocks along the fastest axis can
 *               touch).  On the device, for listed tiles only, dctzhip_decompress_box_nd's index check: a failing tile
 *               reads no AC_exact, the call returns DCTZHIP_E_ARG, the outputs are undefined and the context stays usable.
 * Returns once that check is known, having synchronised the context's stream once.
 * dctzhip_debug_counter 13 / 14 / 15 report the last list call of either kind (this one or dctzhip_decompress_boxes):
 * items of its list, workgroups of its decode launch, the list's bound. */
int dctzhip_decompress_boxes_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                                uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                                const size_t *dims, int dtype, double error_bound, double sf, int mode,
                                int k, const dctzhip_box_item *boxes /* host */);

/* ---- coarse decode: the whole array at reduced resolution -------------------- */
/* An overview of the whole array at 1 / factor of its resolution along every axis, from the low coefficients of every
 * block -- without decoding the array.  For a block of length N (64; 8 or 4 per axis of a tile) with de-quantised
 * coefficients c[0 .. N-1] -- (T)DC, a bin centre or (T)exact, with the QT de-normalisation in QT mode: exactly what
 * every decoder's de-quantise step yields -- the full decoders write
 *     x[m] = sf sum_k alpha_N(k) c[k] cos(pi k (2m + 1) / (2N)),   alpha_N(0) = sqrt(1/N), alpha_N(k > 0) = sqrt(2/N);
 * with K = N / factor the coarse decode writes, for i = 0 .. K-1,
 *     y[i] = sf sum_{k < K} alpha_N(k) c[k] cos(pi k (2i + 1) / (2K)):
 * the part of the reconstruction below frequency K at the centres of the K cells of `factor` elements (the K-point
 * orthonormal DCT-III of sqrt(K/N) c[0 .. K-1]).  The mean of y over a block is the block mean of the full reconstruction;
 * K = 1 gives sf c[0] / sqrt(N).  Tiles use the formula separably along every axis, on the low corner k_a < K of the
 * tile's row-major coefficients.  dctzhip_decompress_coarse and dctzhip_decompress_coarse_nd write the whole array; a window
 * of a TILED array at the same reduced resolution is dctzhip_decompress_coarse_box_nd below, and a part at full resolution
 * is what the box calls are for.  (In flat blocks "coarse" thins the flat index, not the axes of an N-D view: no box there.)
 *
 * dctzhip_decompress_coarse   flat 64-element blocks (dctzhip_compress); factor in {2, 4, 8, 16, 32, 64}.
 *   d_out       receives dctzhip_coarse_len(n, factor) = ceil(n / factor) elements of the data type; block b writes
 *               d_out[b K, b K + K).  The short last block (l = n % 64, not a power-of-two transform) contributes
 *               ceil(l / factor) values: each is the mean of one cell of the values dctzhip_decompress writes for that
 *               block, summed left to right in the data type (starting from the cell's first value) and divided by the
 *               cell's element count -- the last cell may be partial.  These are reproducible bit for bit from the full
 *               decode.
 * dctzhip_decompress_coarse_nd   the tiles of dctzhip_compress_nd; factor in {2, 4, 8} (2-D) or {2, 4} (3-D).
 *   d_out       receives a dense C-order array of extents ceil(dims[i] / factor).  Edge tiles were padded on compress by
 *               repeating the last sample: cells that begin inside the array are written, cells that begin past it are
 *               not.  A cell that straddles the edge is evaluated from the padded tile, i.e. it sees the repeated
 *               samples as well as the array's own.
 * Both:
 *   d_index     dctzhip_ac_index's, of n (flat) or 64 * dctzhip_nd_blocks(ndims, dims) positions.
 *   factor == block edge (64; 8 | 4)   the call reads the DC stream only: d_bin_index, d_ac_exact and d_index may be NULL
 *               -- except for a flat array with n % 64 != 0, whose short block is decoded in full (NULL is refused then).
 *   refusals    before any launch, DCTZHIP_E_ARG for a factor outside the lists above, a null or misaligned pointer (the
 *               rules of dctzhip_decompress_range), a d_out that overlaps an input, and a QT call without a table.  On
 *               the device, for other factors (and the short block's tile): the flags of every tile t must number
 *               idx[t + 1] - idx[t], and idx[t + 1] <= ac_count; a tile that fails reads no AC_exact and the call
 *               returns DCTZHIP_E_ARG, the output is undefined and the context stays usable.
 * Returns once that check is known, as dctzhip_decompress_box does (the call has synchronised the stream).
 * dctzhip_debug_last_kernel(ctx, 1, ...) names the coarse kernel afterwards. */
size_t dctzhip_coarse_len(size_t n, int factor);   /* 0 for a bad factor */
int dctzhip_decompress_coarse(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                              uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                              double error_bound, double sf, int mode, int factor, void *d_out);
int dctzhip_decompress_coarse_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                                 uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                                 const size_t *dims, int dtype, double error_bound, double sf, int mode, int factor,
                                 void *d_out);
/* A box of what dctzhip_decompress_coarse_nd writes: a window at zoom level `factor`.  Everything up to `factor` is that
 * call's (factor in {2, 4, 8} for 2-D, {2, 4} for 3-D); lo / hi are in COARSE coordinates, lo[i] < hi[i] <= ceil(dims[i] /
 * factor).
 *   d_out       receives prod (hi[i] - lo[i]) elements, dense, in C order; each is, bit for bit, the element that
 *               dctzhip_decompress_coarse_nd writes at the same coarse coordinates with the same remaining arguments (EC and
 *               QT, fp32 and fp64, aligned and ragged extents; a cell that straddles a ragged edge keeps that call's rule).
 *   locality    with K = edge / factor, block coordinate b owns the coarse cells [b K, b K + K) per axis: the blocks that
 *               hold box cells are lo[i] / K ... (hi[i] - 1) / K, a box of the row-major block grid.  A stream tile (64
 *               consecutive blocks) is HIT if it holds one of them; candidate tiles run from the first to the last such
 *               block.  Only hit tiles are read and decoded, once each -- their bin ids and DC values, idx[t] and idx[t + 1],
 *               AC_exact[idx[t], idx[t + 1]) -- and nothing outside d_out[0, prod ext) is written.
 *   factor == block edge   the block grid is the output grid: the box is gathered from the DC stream alone ((T)DC * 0.125,
 *               then * sf if sf != 1, as the whole-array call), the DC words from the first to the last block of the box;
 *               d_bin_index, d_ac_exact and d_index may be NULL.
 *   refusals    before any launch, DCTZHIP_E_ARG: what dctzhip_decompress_coarse_nd refuses for ctx, shape, dtype, mode,
 *               factor, the streams, alignment and the QT table; a null lo or hi; a box that is not inside the coarse
 *               extents; a d_out that overlaps what the call may read (the candidate tiles' bin ids, DC values and index
 *               entries and AC_exact[0, ac_count); for factor == block edge the DC words named above).  On the device, for
 *               hit tiles only, the index check of the whole-array call: a failing tile reads no AC_exact, the call returns
 *               DCTZHIP_E_ARG, the output is undefined and the context stays usable.
 * Returns once that check is known, as the box calls do (the call has synchronised the stream).
 * dctzhip_debug_last_kernel(ctx, 1, ...) names the kernel (k_ndcoarse_box<...> | k_ndcoarse_box_dc<...>); dctzhip_debug_counter
 * 11 / 12 report this call too: the workgroups of its launch and its candidate tiles (0 for factor == block edge). */
int dctzhip_decompress_coarse_box_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                                     uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                                     const size_t *dims, int dtype, double error_bound, double sf, int mode, int factor,
                                     const size_t *lo, const size_t *hi, void *d_out);
/* k such boxes of the SAME tiled array at ONE zoom level in one call: what dctzhip_decompress_boxes_nd is to
 * dctzhip_decompress_box_nd.  Everything up to `factor` is dctzhip_decompress_coarse_box_nd's (factor in {2, 4, 8} for 2-D,
 * {2, 4} for 3-D; one factor serves the whole call -- a caller with three levels makes three calls); boxes is a HOST array
 * of 1 <= k <= DCTZHIP_BOXES_MAX items, lo / hi in COARSE coordinates, the first ndims entries are used.  One box table
 * handed over in one transfer, one work list of (box, hit stream tile) pairs built on the device from the boxes of the
 * block grid, one persistent decode launch whose workgroups take list items, and one synchronisation.
 *   boxes[i].d_out  receives exactly the bytes dctzhip_decompress_coarse_box_nd writes for box i with the same remaining
 *               arguments -- the slice of dctzhip_decompress_coarse_nd, bit for bit (EC and QT, fp32 and fp64, aligned and
 *               ragged extents; a cell that straddles a ragged edge keeps the whole-array call's rule).
 *   overlap     boxes may overlap, nest or repeat.  A stream tile hit by m boxes is decoded m times.
 *   locality    the call reads the bin ids, DC values, idx[t], idx[t + 1] and AC_exact[idx[t], idx[t + 1]) of stream tiles
 *               hit by at least one box and nothing else of the streams; it writes nothing outside the k outputs.
 *   factor == block edge   all boxes are gathered from the DC stream alone in one launch, without a list ((T)DC * 0.125,
 *               then * sf if sf != 1); d_bin_index, d_ac_exact and d_index may be NULL.  Per box only the DC words from its
 *               first to its last block count as read.
 *   refusals    before anything is launched or written, all or nothing, DCTZHIP_E_ARG: k < 1, k > DCTZHIP_BOXES_MAX, a null
 *               boxes; what dctzhip_decompress_coarse_box_nd refuses for ctx, shape, dtype, mode, factor, the streams,
 *               alignment and the QT table; for any box what it refuses for lo, hi and d_out (the message names "box i");
 *               an output that overlaps another output or what any box of the call may read (its candidate tiles' bin ids,
 *               DC values and index entries, AC_exact[0, ac_count); for factor == block edge the DC words named above);
 *               for other factors, boxes that may hit more than 2^24 stream tiles in all (the bound of the work list, as
 *               for dctzhip_decompress_boxes_nd).  On the device, for listed tiles only, the index check of the
 *               whole-array call: a failing tile reads no AC_exact, the call returns DCTZHIP_E_ARG, the outputs are
 *               undefined and the context stays usable.
 * Returns once that check is known, having synchronised the context's stream once.
 * dctzhip_debug_counter 13 / 14 / 15 report this call like the other list calls: items of its list, workgroups of its
 * decode launch, the list's bound (factor == block edge: no list, items and bound are 0).  dctzhip_debug_last_kernel(ctx, 1,
 * ...) names the kernel (k_ndcoarse_mbox<T, mode, geometry, K> | k_ndcoarse_mbox_dc<T>). */
int dctzhip_decompress_coarse_boxes_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                                       uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                                       const size_t *dims, int dtype, double error_bound, double sf, int mode, int factor,
                                       int k, const dctzhip_box_item *boxes /* host */);

/* ---- tile summaries: verify and survey without writing the decode ----------- */
/* Two questions about a compressed array that need no reconstruction in memory: how far is it from the original, and where
 * in it is anything worth decoding.  One record per stream tile (4096 elements, one index entry) of what dctzhip_decompress
 * would write there, reduced in registers; with the original at hand (d_ref) also of the error, tile by tile: an error map.
 * It reports the bound actually reached and promises none.  Flat 64-element blocks (the streams of dctzhip_compress, fp32
 * and fp64, EC and QT, the short last block included); the streams of dctzhip_compress_nd carry edge padding that has to be
 * kept out of every reduction, which needs the geometry: they have dctzhip_tile_summary_nd below.
 *   r           the elements dctzhip_decompress writes for the same arguments, bit for bit.
 *   rmin, rmax, xmin, xmax, emax   exact.  Minima and maxima pass a NaN over (fmin / fmax, as dctzhip_psnr_terms does); a tile
 *               of nothing but NaNs reports the starting pair rmin = +DBL_MAX, rmax = -DBL_MAX.
 *   rsum, rsq, esq   summed in double, unfused; they carry a NaN.  The order of a tile's sum is fixed: the same call gives
 *               the same bytes in every record every time, on every context, whatever grid is launched.  The r-fields with
 *               and without d_ref may differ in their last digits (two orders).
 *   d_ref       (or NULL) the ORIGINAL, n elements of dtype, 16-byte aligned -- what was handed to compress, not its
 *               d_scaled output.  NULL: xmin, xmax, emax and esq are 0.
 *   d_tiles     (or NULL) receives dctzhip_summary_tiles(n) records, 8-byte aligned; NULL: they live in scratch of the
 *               context and only *total is reported.  At least one of d_tiles and total must be given.
 *   total       (or NULL, HOST) the records joined: extremes over all records, sums added from the records in a fixed order
 *               that depends on the tile count alone (a reduction kernel of its own, no atomics).  With d_ref, xmin, xmax
 *               and emax equal dctzhip_psnr_terms' out[0], out[1], out[2] exactly, and
 *               20 log10((xmax - xmin) / sqrt(esq / n)) is calc_psnr.
 *   refusals    before any launch, DCTZHIP_E_ARG: the pointer and alignment rules of dctzhip_decompress_range, a d_ref that
 *               is not 16-byte aligned, a d_tiles that is not 8-byte aligned or overlaps any input, both d_tiles and total
 *               NULL, a QT call without a table, n == 0.  On the device: the flags of every tile t must number
 *               idx[t + 1] - idx[t], and idx[t + 1] <= ac_count; a tile that fails reads no AC_exact and the call returns
 *               DCTZHIP_E_ARG, the records are undefined and the context stays usable.
 * Returns once that check is known, as dctzhip_decompress_box does (the call has synchronised the stream).
 * dctzhip_debug_last_kernel(ctx, 1, ...) names the summary kernel afterwards. */
typedef struct {             /* one per tile: elements [4096 t, min(4096 (t + 1), n)); 64 bytes */
  double rmin, rmax;         /* min / max of r, the elements dctzhip_decompress writes (exact) */
  double rsum, rsq;          /* sum (double)r, sum (double)r * (double)r */
  double xmin, xmax;         /* min / max of the original        (d_ref only, else 0) */
  double emax, esq;          /* max |x - r|, sum (double)(e * e), e = x - r and e * e taken in the data type, as k_psnr does (d_ref only, else 0) */
} dctzhip_tile_summary_t;
size_t dctzhip_summary_tiles(size_t n);     /* ceil(n / 4096) */
int dctzhip_tile_summary(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                         uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                         double error_bound, double sf, int mode, const void *d_ref /* or NULL */,
                         dctzhip_tile_summary_t *d_tiles /* or NULL */, dctzhip_tile_summary_t *total /* host, or NULL */);

/* dctzhip_tile_summary for the streams of dctzhip_compress_nd (8 x 8 / 4 x 4 x 4 tiles): the same record, per stream tile, over
 * the array's own elements.  Streams, ac_count, qtable_host, ndims, dims, dtype, error_bound, sf and mode are
 * dctzhip_decompress_nd's; d_index is dctzhip_ac_index's over the 64 * dctzhip_nd_blocks(ndims, dims) stream positions, as
 * for dctzhip_fixup_build_nd.
 *   positions   as in dctzhip_fixup_build_nd: position q belongs to block q >> 6 (row-major over the block grid) at in-block
 *               place q & 63 (row-major in the tile); it is REAL iff every coordinate is below its extent.  Record t covers
 *               the real positions among [4096 t, min(4096 (t + 1), 64 nblk)); every block holds a real position, so no
 *               record is empty.  There are dctzhip_summary_tiles(64 * nblk) records.  A padded position enters no field,
 *               and the original is never read there, nor outside d_ref[0, prod dims).
 *   r           the element dctzhip_decompress_nd writes at the same coordinates, bit for bit.
 *   fields      as above: extremes exact and NaN-passing (a tile of nothing but NaNs: +DBL_MAX / -DBL_MAX), rsum, rsq and esq
 *               summed in double, unfused, NaN-carrying; e = x - r and e * e in the data type; without d_ref the last four
 *               fields are +0.0.
 *   order       of a record's sums: fixed by dims and the geometry (e = 8 | 4 the tile edge), independent of the grid
 *               launched, the context and the call count -- the same call gives the same bytes every time.
 *               Without d_ref: lane b of a wave takes block b of the stream tile, places j = 0 .. 63 in order, into four
 *               running sums by j mod 4, joined (0 + 1) + (2 + 3).  With d_ref: lane l takes, for s = 0 .. e - 1 and in-block
 *               row i = 0 .. 64 / e - 1, in-row offset l mod e of the tile's block l / e + (64 / e) s, into two running sums
 *               by i mod 2, joined 0 + 1.  Either way a position that is not real adds nothing, and the 64 lanes join in a
 *               butterfly: partners 32, 16, 8, 4, 2, 1 lanes apart.  The r-fields with and without d_ref may differ in
 *               their last digits (two orders).
 *   d_ref       (or NULL) the ORIGINAL in C order, prod dims elements of dtype, aligned to its elements (the rows of a
 *               ragged array are not 16-byte aligned, so nothing more is asked).
 *   d_tiles, total   as above; total joins the records with the same reduction kernel, in an order that depends on the tile
 *               count alone.  With d_ref, total's xmin, xmax and emax equal out[0 .. 2] of dctzhip_psnr_terms over the
 *               original and dctzhip_decompress_nd's output exactly, and 20 log10((xmax - xmin) / sqrt(esq / prod dims)) is
 *               calc_psnr.
 *   refusals    before any launch, DCTZHIP_E_ARG: what dctzhip_fixup_build_nd refuses for the same arguments (ndims not 2
 *               or 3, a zero extent, null or misaligned stream pointers, QT without a table), both d_tiles and total NULL, a
 *               d_ref that is not aligned to its elements, a d_tiles that is not 8-byte aligned or overlaps an input.  On the
 *               device: the index check above; a tile that fails reads no AC_exact, the call returns DCTZHIP_E_ARG and the
 *               context stays usable.
 * Host-synchronous on return; dctzhip_debug_last_kernel(ctx, 1, ...) names the summary kernel afterwards. */
int dctzhip_tile_summary_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                            uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                            const size_t *dims, int dtype, double error_bound, double sf, int mode,
                            const void *d_ref /* or NULL */, dctzhip_tile_summary_t *d_tiles /* or NULL */,
                            dctzhip_tile_summary_t *total /* host, or NULL */);

/* ---- point-wise error bound: a correction list beside the streams ------------ */
/* DCTZ bounds the error of every COEFFICIENT; an element's error can reach about twice error_bound * sf.  The correction list
 * repairs that without touching the streams: it names every element whose reconstruction misses the original by more than a
 * bound and keeps the original's value for it.  Applied to the output of any decode of the same streams -- whole array,
 * range, box -- it makes that output bounded.  Flat 64-element blocks (the streams of dctzhip_compress, fp32 and fp64, EC
 * and QT, the short last block included), as for dctzhip_tile_summary; the streams of dctzhip_compress_nd have the _nd pair
 * further down.
 *   x           the ORIGINAL, n elements of dtype: what was handed to compress, not its d_scaled output.
 *   r           the elements dctzhip_decompress writes for the same arguments, bit for bit.
 *   bound       an absolute bound b >= 0 in the data's units, taken as (T)b in the data type T (round to nearest).
 *   listed      element i is listed iff !(fabs(x[i] - r[i]) <= (T)b), the difference taken in the data type.  A NaN on either
 *               side therefore lists the element: the 63 finite neighbours a NaN drags down with its block are listed and
 *               restored, the NaN itself is listed and stays a NaN.  The list stores x[i] itself, bit for bit.
 *   layout      with m = dctzhip_fixup_tiles(n) tiles of 4096 elements (the tiles of the exception index):
 *                 fix_start[0 .. m]   uint32: listed elements in the tiles in front of t; fix_start[m] == count
 *                 fix_off[count]      uint16: offset in the tile (0 .. 4095), strictly ascending inside a tile
 *                 fix_val[count]      elements of the data type
 *               entries run tile after tile: a range or box apply touches only its own tiles' entries.
 *   guarantee   after apply every element of the output either has the bits of x[i] or satisfies
 *               fabs(x[i] - out[i]) <= (T)b.
 *
 * dctzhip_fixup_build: streams, alignment rules, overlap refusals and the in-kernel index check are dctzhip_tile_summary's (a
 * tile whose flags disagree with the index reads no AC_exact; the call returns DCTZHIP_E_ARG, the outputs are undefined and
 * the context stays usable).
 *   d_ref       the original, 16-byte aligned.
 *   d_fix_start m + 1 entries, 4-byte aligned; always complete on DCTZHIP_OK and DCTZHIP_E_SPACE.
 *   d_fix_off, d_fix_val   `capacity` entries each (2-byte / element aligned), or both NULL: the count-only form ("what
 *               would bound b cost?"), which returns DCTZHIP_OK.
 *   count       (HOST) always reported on DCTZHIP_OK and DCTZHIP_E_SPACE.  If *count > capacity the call returns
 *               DCTZHIP_E_SPACE and nothing is written to d_fix_off / d_fix_val.
 *   refusals    before any launch, DCTZHIP_E_ARG: what dctzhip_tile_summary refuses; d_ref or count NULL; a bound that is
 *               negative, NaN or infinite; d_fix_start NULL or misaligned; exactly one of d_fix_off / d_fix_val NULL, or one
 *               misaligned; an output that overlaps an input or another output.
 * The same call gives the same bytes every time, on every context, whatever grid is launched.  Host-synchronous like
 * dctzhip_tile_summary; dctzhip_debug_last_kernel(ctx, 1, ...) names the mark kernel afterwards.
 *
 * dctzhip_fixup_apply: d_out is the dense C-order box lo[i] <= c[i] < hi[i] of the array seen as ndim-dimensional (1 ..
 * DCTZHIP_BOX_MAXDIM, prod dims == n) -- exactly what dctzhip_decompress_box or dctzhip_decompress_boxes wrote; a range
 * [lo, hi) is the 1-D case, the whole array ndim = 1, lo = 0, hi = n.  Only the tiles between the box's first and its last
 * element are visited.
 *   refusals    before any launch, DCTZHIP_E_ARG: the box rules of dctzhip_decompress_box; d_fix_start or d_out NULL or
 *               misaligned (4 bytes / element size); count > n; with count > 0 a NULL or misaligned d_fix_off (2 bytes) /
 *               d_fix_val (element size); d_out overlapping the list.  On the device the list is untrusted input: a visited
 *               tile is refused, by plain comparisons made before any store of that tile, for fix_start[t + 1] <
 *               fix_start[t], fix_start[t + 1] > count, an offset beyond the tile's elements, or offsets that are not
 *               strictly ascending; every call is refused for fix_start[m] != count.  The call then returns DCTZHIP_E_ARG,
 *               d_out is undefined inside its box, nothing outside it is ever written, and the context stays usable.
 * Host-synchronous; dctzhip_debug_last_kernel(ctx, 1, ...) names the apply kernel afterwards. */
size_t dctzhip_fixup_tiles(size_t n);       /* ceil(n / 4096) */
int dctzhip_fixup_build(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                        uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, size_t n, int dtype,
                        double error_bound, double sf, int mode, const void *d_ref, double bound, uint32_t *d_fix_start,
                        uint16_t *d_fix_off /* or NULL */, void *d_fix_val /* or NULL */, uint32_t capacity,
                        uint32_t *count /* host */);
int dctzhip_fixup_apply(dctzhip_ctx *ctx, const uint32_t *d_fix_start, const uint16_t *d_fix_off, const void *d_fix_val,
                        uint32_t count, size_t n, int dtype, int ndim, const size_t *dims, const size_t *lo,
                        const size_t *hi, void *d_out);

/* The correction list of an array compressed in 8 x 8 / 4 x 4 x 4 tiles: the streams of dctzhip_compress_nd, fp32 and fp64,
 * EC and QT, 2-D and 3-D, aligned and ragged extents alike.  The flat list's contract with stream positions in place of
 * elements:
 *   positions   the streams cover 64 nblk positions, nblk = dctzhip_nd_blocks(ndims, dims).  Position q belongs to block
 *               B = q >> 6, numbered row-major over the tile grid; its in-block place is j = q & 63, row-major inside the
 *               tile: j = 8 r + c in 2-D, j = 16 z + 4 y + x in 3-D.  Its coordinate along axis a is e B_a + j_a with e = 8 in
 *               2-D and 4 in 3-D.  A position is REAL iff every coordinate is below dims[a]; the others are the edge padding.
 *   x           the ORIGINAL array, not d_scaled.
 *   r           what dctzhip_decompress_nd writes at the same coordinates, bit for bit.
 *   bound       b >= 0, taken as (T)b.
 *   listed      a real position is listed iff !(fabs(x - r) <= (T)b), the difference taken in T.  A padded position is never
 *               listed, and the original is never read there.  A NaN on either side lists the position: a NaN in the original
 *               lists every real position of its tile and stays a NaN.
 *   layout      with m = dctzhip_fixup_tiles(64 nblk) stream tiles of 4096 positions (the tiles of the exception index and of
 *               dctzhip_decompress_box_nd's hit test):
 *                 fix_start[0 .. m]   uint32; fix_start[m] == count
 *                 fix_off[count]      uint16: q & 4095, strictly ascending inside a tile
 *                 fix_val[count]      T: x itself, bit for bit
 *               The bytes depend on the streams, the original and b alone, never on the grid.
 *   guarantee   after apply every element of the output has the original's bits or lies within (T)b of it.
 *
 * dctzhip_fixup_build_nd: d_ref is the original in its own C-order layout, prod dims elements, 16-byte aligned; it is read in
 * place, for ragged extents too.  The count-only form (d_fix_off and d_fix_val NULL), DCTZHIP_E_SPACE, "count always
 * reported" and the host-synchronous return are dctzhip_fixup_build's, and so are its refusals, with the shape rules of
 * dctzhip_decompress_nd in place of the rules for n and the span and overlap checks made over the sizes above.  The in-kernel
 * index check is the box decoder's: a tile whose flags disagree with the index reads no AC_exact, and the call returns
 * DCTZHIP_E_ARG.  dctzhip_debug_last_kernel(ctx, 1, ...) names the mark kernel afterwards.
 *
 * dctzhip_fixup_apply_nd: d_out is the dense C-order box lo <= c < hi of the array -- exactly what dctzhip_decompress_box_nd
 * wrote, or dctzhip_decompress_nd for lo = 0, hi = dims.  Only the candidate stream tiles are visited, from the first to the
 * last block that meets the box; an entry whose coordinates lie outside the box is passed over.
 *   refusals    before any launch, DCTZHIP_E_ARG: the shape and box rules of dctzhip_decompress_box_nd; d_fix_start or d_out
 *               NULL or misaligned (4 bytes / element size); count > prod dims; with count > 0 a NULL or misaligned d_fix_off
 *               / d_fix_val; d_out overlapping the list.  On the device the list is untrusted input: a visited tile is refused,
 *               by plain comparisons made before any store of that tile, for dctzhip_fixup_apply's reasons (table not
 *               monotone, more entries than count, more entries than the tile holds, offsets not strictly ascending), for an
 *               entry in a block >= nblk and for an entry at a padded position; every call is refused for fix_start[m] !=
 *               count.  The call then returns DCTZHIP_E_ARG, d_out is undefined inside its box, nothing outside it is ever
 *               written, and the context stays usable.
 * Host-synchronous; dctzhip_debug_last_kernel(ctx, 1, ...) names the apply kernel afterwards. */
int dctzhip_fixup_build_nd(dctzhip_ctx *ctx, const void *d_bin_index, const float *d_dc, const float *d_ac_exact,
                           uint32_t ac_count, const uint32_t *d_index, const void *qtable_host, int ndims,
                           const size_t *dims, int dtype, double error_bound, double sf, int mode, const void *d_ref,
                           double bound, uint32_t *d_fix_start, uint16_t *d_fix_off /* or NULL */,
                           void *d_fix_val /* or NULL */, uint32_t capacity, uint32_t *count /* host */);
int dctzhip_fixup_apply_nd(dctzhip_ctx *ctx, const uint32_t *d_fix_start, const uint16_t *d_fix_off,
                           const void *d_fix_val, uint32_t count, int ndims, const size_t *dims, int dtype,
                           const size_t *lo, const size_t *hi, void *d_out);

/* ---- missing values: a mask beside the streams, the holes filled on compress ------------ */
/* Fields with missing values (1e36 over land, NaN) ruin the codec as they are: sf is taken over every element, a NaN costs
 * its 64-element block, an infinity the array.  The mask layer keeps one bit per element beside the streams, compresses a
 * FILLED array whose holes hold copies of their valid neighbours, and writes the caller's fill value back after any decode.
 * No compress or decode kernel and no stream byte changes.  These three calls fill inside flat 64-element blocks; arrays
 * compressed in tiles have dctzhip_mask_build_nd / dctzhip_compress_masked_nd below, and share dctzhip_mask_apply.
 *   missing     element x (data type T) is missing iff a selected test holds, made in T:
 *                 DCTZHIP_MISS_NAN      x != x (signalling NaNs too)
 *                 DCTZHIP_MISS_INF      fabs(x) == inf
 *                 DCTZHIP_MISS_VALUE    x == (T)value (-0.0 matches 0.0; a NaN value is refused: use MISS_NAN)
 *                 DCTZHIP_MISS_ABS_GE   fabs(x) >= (T)limit (limit finite and > 0)
 *               every other element is valid.
 *   fill rule   blocks are the codec's: elements [64 b, 64 b + 64), the short last block has n % 64.  A missing element of
 *               block B takes the value of the nearest valid element before it in B; else (a leading gap) the first valid
 *               element of B; else (no valid element in B) +0.0.  Valid elements keep their bits; every filled value is a
 *               copy of one, so the filled array has no missing element and its max|x| is the valid data's; so is its
 *               min|x|, unless a block without a valid element brings in its +0.0.  (MISS_VALUE with value 0 calls that +0.0
 *               missing again: the one case in which the fill is not idempotent.)
 *   mask        dctzhip_mask_words(n) = ceil(n / 64) words of 64 bits: bit i & 63 of word i >> 6 is 1 iff element i is
 *               missing.  Build writes the bits at positions >= n as 0; apply ignores them.
 *
 * dctzhip_mask_build: one pass over the array -- the mask, the count and (unless d_filled is NULL) the filled copy.
 *   d_filled    NULL, exactly d_in (in place) or disjoint from it.
 *   count       (HOST) the number of missing elements.
 *   refusals    before any launch, DCTZHIP_E_ARG: ctx, d_in, miss, d_mask or count NULL; n == 0 or a bad dtype; flags of 0 or
 *               with unknown bits; MISS_VALUE with a NaN value; MISS_ABS_GE with a limit that is not finite and > 0; d_in or
 *               d_filled not 16-byte aligned, d_mask not 8-byte aligned; d_filled overlapping d_in partly; the mask
 *               overlapping an array.
 * The same call gives the same bytes every time, on every context, whatever grid is launched.  Host-synchronous like
 * dctzhip_fixup_build; dctzhip_debug_last_kernel(ctx, 1, ...) names the kernel afterwards.
 *
 * dctzhip_compress_masked: dctzhip_mask_build followed by dctzhip_compress(ctx, filled, n, dtype, error_bound, mode,
 * d_bin_index, d_dc, d_ac_exact, NULL, NULL, info): streams and *info are bit for bit that call's.  d_in is not modified.
 *   d_filled    n elements that receive the filled array -- the reference to hand dctzhip_tile_summary and
 *               dctzhip_fixup_build -- or NULL: the context keeps the copy in scratch of its own.
 *   refusals    those of the two calls, all made before any launch.
 *
 * dctzhip_mask_apply: d_out is the dense C-order box of dctzhip_fixup_apply (a range is the 1-D case, the whole array ndim = 1,
 * lo = 0, hi = n).  Every box element whose bit is set receives (T)fill (a NaN fill: a quiet NaN, its payload not pinned);
 * nothing else is written, inside the box or outside it; only the mask words the box touches are read.  Any bit pattern is a
 * valid mask.
 *   refusals    before any launch, DCTZHIP_E_ARG: the box rules of dctzhip_decompress_box; d_mask or d_out NULL or misaligned
 *               (8 bytes / element size); d_out overlapping the mask.
 * Host-synchronous; dctzhip_debug_last_kernel(ctx, 1, ...) names the apply kernel afterwards.
 *
 * Composed guarantee: compress with dctzhip_compress_masked, build the correction list against d_filled, decode by any whole,
 * range or box path, run dctzhip_fixup_apply, then dctzhip_mask_apply.  Every valid element then has the original's bits or
 * lies within the list's bound of it, and every missing element has the fill's bits. */
#define DCTZHIP_MISS_NAN     1u   /* x != x (signalling NaNs too) */
#define DCTZHIP_MISS_INF     2u   /* fabs(x) == inf */
#define DCTZHIP_MISS_VALUE   4u   /* x == (T)value: -0.0 matches 0.0; a NaN value is refused, use MISS_NAN */
#define DCTZHIP_MISS_ABS_GE  8u   /* fabs(x) >= (T)limit; limit finite and > 0 */
typedef struct { unsigned flags; double value; double limit; } dctzhip_missing;
size_t dctzhip_mask_words(size_t n);
int dctzhip_mask_build(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, const dctzhip_missing *miss,
                       uint64_t *d_mask, void *d_filled /* NULL, == d_in, or disjoint */, uint64_t *count /* host */);
int dctzhip_mask_apply(dctzhip_ctx *ctx, const uint64_t *d_mask, size_t n, int dtype, double fill, int ndim,
                       const size_t *dims, const size_t *lo, const size_t *hi, void *d_out);
int dctzhip_compress_masked(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, double error_bound, int mode,
                            const dctzhip_missing *miss, void *d_bin_index, float *d_dc, float *d_ac_exact,
                            uint64_t *d_mask, void *d_filled /* or NULL: context scratch, kept */, dctzhip_cinfo *info,
                            uint64_t *count /* host */);

/* Missing values of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (dctzhip_compress_nd), fp32 and fp64, 2-D and 3-D, aligned
 * and ragged extents alike.  The tests for "missing" are the ones above.
 *   positions   those of dctzhip_fixup_build_nd: block B numbered row-major over the tile grid, the in-block place j = 8 r + c
 *               in 2-D and j = 16 z + 4 y + x in 3-D; a position is REAL iff every coordinate is below dims[a].
 *   fill rule   a real missing position of tile B takes the value of the nearest real valid position before it in B, in
 *               ascending j; else the tile's first real valid position; else +0.0.  Padded positions are neither valid nor
 *               missing and are never read or written.  Valid elements keep their bits; every filled value is a copy, moved
 *               as a bit pattern (a signalling NaN among valid data keeps its bits).  The edge padding of dctzhip_compress_nd
 *               (repeat the last sample) then acts on the filled array as on any array.
 *   mask        exactly the flat layer's mask of the array seen as n = prod dims elements in C order -- byte for byte what
 *               dctzhip_mask_build(d_in, n, ..., d_filled = NULL) writes -- so dctzhip_mask_apply serves tiled arrays as it is.
 *
 * dctzhip_mask_build_nd: one pass over the array -- the mask, the count and (unless d_filled is NULL) the filled copy, in the
 * array's own C-order layout.  d_filled: NULL, exactly d_in (in place) or disjoint from it.
 *   refusals    before any launch, DCTZHIP_E_ARG: the shape rules of dctzhip_compress_nd (which keep prod dims below 2^31);
 *               the rules of dctzhip_mask_build for NULL pointers, dtype, flags, a NaN value and a bad limit; d_in or d_filled
 *               not 16-byte aligned, d_mask not 8-byte aligned; d_filled overlapping d_in partly; the mask overlapping an
 *               array.  The context stays usable.
 * The same call gives the same bytes every time, on every context, whatever grid is launched.  Host-synchronous;
 * dctzhip_debug_last_kernel(ctx, 1, ...) names the kernel afterwards.
 *
 * dctzhip_compress_masked_nd: dctzhip_mask_build_nd followed by dctzhip_compress_nd(ctx, filled, ndims, dims, dtype,
 * error_bound, mode, d_bin_index, d_dc, d_ac_exact, NULL, info): streams and *info are bit for bit that call's.  d_in is not
 * modified.  d_filled: prod dims elements that receive the filled array -- the reference to hand dctzhip_fixup_build_nd -- or
 * NULL: the context keeps the copy in scratch of its own.  Refusals: those of the two calls, all made before any launch.
 *
 * Composed guarantee: dctzhip_compress_masked_nd; dctzhip_fixup_build_nd against d_filled; dctzhip_decompress_nd or
 * dctzhip_decompress_box_nd; dctzhip_fixup_apply_nd; dctzhip_mask_apply(d_mask, prod dims, dtype, fill, ndims, dims, lo, hi,
 * d_out).  Every valid element then has the original's bits or lies within the list's bound of it, and every missing element
 * has the fill's bits. */
int dctzhip_mask_build_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype,
                          const dctzhip_missing *miss, uint64_t *d_mask,
                          void *d_filled /* NULL, == d_in, or disjoint */, uint64_t *count /* host */);
int dctzhip_compress_masked_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype,
                               double error_bound, int mode, const dctzhip_missing *miss, void *d_bin_index, float *d_dc,
                               float *d_ac_exact, uint64_t *d_mask, void *d_filled /* or NULL: context scratch, kept */,
                               dctzhip_cinfo *info, uint64_t *count /* host */);

/* ---- transform only ------------------------------------------------------ */
/* Batched drop-in for dct_init + per-block dct_fftw / ifft_idct (+ the
 * remainder-length re-init), dct.h:17-27 as driven by dct-test.c:81-89, 144-152:
 * forward (inverse = 0) or inverse (inverse = 1) orthonormal DCT of every
 * 64-element block of d_in, last block of length n % 64 if non-zero. */
int dctzhip_dct_blocks(dctzhip_ctx *ctx, const void *d_in, void *d_out, size_t n,
                       int dtype, int inverse);

/* ---- multi-GPU: gather of the pre-zlib streams ------------------------------ */
/* Shards are independent dctz_compress calls (own sf, own header; nothing in the reference couples them,
 * dctz-comp-lib.c:186): one process or thread per GPU, one context each, no data-path collective.  The one exchange
 * step is bringing the three streams of every shard to the rank whose host runs the zlib tail
 * (dctz-comp-lib.c:620-760).  It runs over RCCL (loaded with dlopen on first use: single-GPU users need no RCCL):
 * an all-gather of three 64-bit sizes per rank, then grouped point-to-point sends straight to the root, so that
 * all seven inbound xGMI links of the root carry data at once (a ring would be bound by one link).
 *   dctzhip_comm_unique_id   rank 0 makes the 128-byte id and hands it to the other ranks (file, socket, MPI, ...)
 *   dctzhip_comm_create      collective over all ranks; the communicator lives in the context
 *   dctzhip_comm_sizes       collective: sizes[3 r .. 3 r + 2] = {n, nblk, cnt} of rank r, on every rank (host memory)
 *   dctzhip_comm_gather      collective: on `root`, d_*_all receive the streams of all ranks back to back in rank
 *                            order (offsets = prefix sums of `sizes`; root's own streams are copied); the other
 *                            ranks pass NULL.  Synchronous with respect to the host on return. */
#define DCTZHIP_COMM_ID_BYTES 128
int dctzhip_comm_unique_id(void *id_out);
int dctzhip_comm_create(dctzhip_ctx *ctx, int rank, int world, const void *id);
int dctzhip_comm_destroy(dctzhip_ctx *ctx);
int dctzhip_comm_sizes(dctzhip_ctx *ctx, uint64_t n, uint64_t cnt, uint64_t *sizes);
int dctzhip_comm_gather(dctzhip_ctx *ctx, int root, const void *d_bin, const float *d_dc, const float *d_ac,
                        const uint64_t *sizes, void *d_bin_all, float *d_dc_all, float *d_ac_all);

/* ---- harness metric ------------------------------------------------------- */
/* The reductions of calc_psnr (util.c:54-104) over device-resident arrays:
 * out[0] = min x, out[1] = max x (util.c:61-66 / :77-82), out[2] = max |x - r|,
 * out[3] = sum (x - r)^2 with the difference and its square taken in the data type
 * (util.c:67-73 / :83-89).  The sum is a tree reduction: its last digits differ from
 * the reference's serial loop (relative 1e-15), min / max / maxdiff are exact. */
int dctzhip_psnr_terms(dctzhip_ctx *ctx, const void *d_x, const void *d_r, size_t n, int dtype, double out[4]);

/* ---- rate-distortion probe and target-PSNR compression (EC mode) --------------------------------------------------- */
/* Which error bound does an array need?  The reference's answer is a sweep: the whole compressor, a decode and calc_psnr
 * once per bound (tests/test-dctz.sh, zc-patches/zc-ratedistortion.sh over errBounds.cfg).  The probe reads the array ONCE,
 * scales and transforms every block as dctzhip_compress does, and bins the coefficients against up to DCTZHIP_RD_MAXK
 * bounds in registers.  Per bound it gives the exact count of coefficients stored exactly and the squared error of the
 * reconstruction predicted from the coefficients' own errors (the transform is orthonormal; the decoder's value of every
 * coefficient -- bin centre, float-truncated exact value, float-truncated DC -- is known when it is binned).  The
 * prediction misses the measured sum only by the rounding of the inverse transform and of the de-scaling.
 *   error_bounds  k bounds, 1 <= k <= DCTZHIP_RD_MAXK, any order, repeats allowed; each >= 1e-6 (else DCTZHIP_E_BOUND)
 *   pts           k results, pts[i] for error_bounds[i]; a bound's result does not depend on the other bounds of the call
 *   range         (or NULL) min x and max x, calc_psnr's range (util.c:61-66; = dctzhip_psnr_terms' out[0], out[1])
 * d_in (16-byte aligned) is not modified.  Host-synchronous on return.  Sums are bitwise reproducible from run to run. */
#define DCTZHIP_RD_MAXK 16
#define DCTZHIP_RD_HEADER_BYTES 56   /* struct header of the EC container (dctz.h:96-119) */
typedef struct {
  double error_bound;
  uint64_t cnt;        /* tot_AC_exact_count dctzhip_compress would report at this bound (exact) */
  double sse;          /* predicted sum (x - x')^2 of the reconstruction, data units (sf^2 * sum err^2) */
  double psnr;         /* predicted calc_psnr: 20 log10((max - min) / sqrt(sse / n)) */
  uint64_t raw_bytes;  /* pre-zlib bytes: n + 4 nblk + 4 cnt + DCTZHIP_RD_HEADER_BYTES (exact; zlib's output is not predicted) */
} dctzhip_rd_point;
int dctzhip_rd_probe(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, int k, const double *error_bounds,
                     dctzhip_rd_point *pts, double range[2]);
/* Compression to a target PSNR.  Deterministic contract:
 *   grid      candidate bounds G = {m * 10^e : m in {1, 1.25, 1.5, 2, 2.5, 3, 4, 5, 6, 8}, e = -6 .. -1} u {1}: 61 points, each
 *             the double nearest to the decimal value (strtod of "1.25e-3", ...)
 *   probes    call 1 probes the decade points 1e-6, 1e-5, ..., 1 and takes the largest whose predicted PSNR >= target; call 2
 *             probes the 9 points of G above that decade point and takes the largest whose prediction >= target (else the
 *             decade point)
 *   compress  the chosen bound goes through the ordinary dctzhip_compress: the streams and *info are bit for bit those of
 *             dctzhip_compress(d_in, ..., *error_bound_used, DCTZHIP_EC, ..., d_scaled = NULL, d_coef = NULL)
 *   measure   the streams are decoded into scratch of the context (n elements of the data type: a device buffer kept for
 *             later calls) and the PSNR is measured with dctzhip_psnr_terms' reductions -> *psnr_measured
 *   step down a measured PSNR under the target moves to the next smaller point of G and repeats (debug counter 10 counts
 *             these); so a rounding-level miss of the prediction costs time, never the target
 *   guarantee on DCTZHIP_OK the returned streams decode to a measured PSNR >= target_psnr
 *   refusals  before anything is written: no point of G is predicted to reach the target -> DCTZHIP_E_BOUND; a constant
 *             array (max == min), a non-finite min / max or a NaN in the array (PSNR undefined), a non-finite target ->
 *             DCTZHIP_E_ARG.  (Should even 1e-6 measure under the target after the prediction reached it, the call returns
 *             DCTZHIP_E_BOUND with the streams of 1e-6 written.)
 *   buffers   as dctzhip_compress's (no scaled copy, no coefficient tap): overlaps are refused with DCTZHIP_E_ARG.
 * Host-synchronous on return.  (tests) dctzhip_debug_knob(ctx, 3, f) divides every predicted SSE by f (the step-down path
 * on purpose); f <= 1 switches it off. */
int dctzhip_compress_psnr(dctzhip_ctx *ctx, const void *d_in, size_t n, int dtype, double target_psnr,
                          void *d_bin_index, float *d_dc, float *d_ac_exact, dctzhip_cinfo *info,
                          double *error_bound_used, double *psnr_measured);
/* The same two calls for an array compressed in 8 x 8 (ndims = 2) or 4 x 4 x 4 (ndims = 3) tiles: whatever
 * dctzhip_compress_nd accepts, aligned and ragged extents alike, fp32 and fp64, EC.  d_in is the array itself in C order
 * (16-byte aligned, not modified), read in place: one pass, the tiles scaled by the sf of the array's own statistics and
 * put through the separable transform as dctzhip_compress_nd does it, then the flat probe's work per coefficient and bound.
 *   cnt        exactly the info.cnt dctzhip_compress_nd reports at that bound (in place or through its gather pass)
 *   sse        the predicted sum (x - x')^2 over the array's own prod dims elements, x' what dctzhip_decompress_nd writes.
 *              The edge padding of the streams enters no field: orthonormality gives the error over all 64 places of a tile,
 *              and for the tiles that hang over an extent the share of their padded places -- the inverse transform of the
 *              coefficients' errors, squared there, exact up to that transform's rounding -- is taken out again
 *   psnr       from min, max, sse and prod dims
 *   raw_bytes  64 nblk + 4 nblk + 4 cnt + DCTZHIP_RD_HEADER_BYTES + 16 (the "DZND" trailer), nblk = dctzhip_nd_blocks
 *   range      min x and max x of the array (= dctzhip_psnr_terms' out[0], out[1])
 * Bounds, k, reproducibility, independence of the other bounds and debug knob 3 are dctzhip_rd_probe's. */
int dctzhip_rd_probe_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype, int k,
                        const double *error_bounds, dctzhip_rd_point *pts, double range[2]);
/* dctzhip_compress_psnr's contract word for word, the search itself being one function for both layouts: the same grid and
 * probes (dctzhip_rd_probe_nd), the streams and *info bit for bit those of dctzhip_compress_nd(d_in, ndims, dims, ...,
 * *error_bound_used, DCTZHIP_EC, ..., d_scaled = NULL), decoded with dctzhip_decompress_nd into the context's scratch
 * and measured with dctzhip_psnr_terms over the prod dims elements; the same step down, guarantee and refusals.  Buffers
 * as dctzhip_compress_nd's (64 nblk bytes, nblk floats, 64 nblk floats); overlaps are refused with DCTZHIP_E_ARG. */
int dctzhip_compress_psnr_nd(dctzhip_ctx *ctx, const void *d_in, int ndims, const size_t *dims, int dtype,
                             double target_psnr, void *d_bin_index, float *d_dc, float *d_ac_exact,
                             dctzhip_cinfo *info, double *error_bound_used, double *psnr_measured);

/* ---- entropy stage on the GPU -------------------------- */
/* Replaces the reference's zlib tail on the compress side -- deflateInit / deflate of bin_index, DC and AC_exact on
 * three host threads, dctz-comp-lib.c:620-732 -- with kernels: every section becomes ONE standard zlib stream
 * (RFC 1950 frame, RFC 1951 blocks) in device memory, which the reference's reader inflates unchanged
 * (dctz-decomp-lib.c:244-322).  Compressed BYTES differ from zlib's (dynamic-Huffman blocks of 16 KiB of input with
 * matches at a fixed set of distances; sizes within a few per cent of zlib level 6 on DCTZ streams), inflated CONTENT
 * is identical.
 *   nsec      sections of this call (<= 8); they share scratch and run one after the other on the context's stream
 *   d_src[i]  n[i] bytes, device (4-byte alignment gives the fast load path)
 *   d_dst[i]  cap[i] >= dctzhip_deflate_bound(n[i]) bytes, device
 *   out_len   stream lengths; the call returns after the stream has drained (it needs them on the host)
 *   chunk_sizes  NULL, or per section a host array of ceil(n[i] / dctzhip_deflate_chunk_bytes()) entries (or NULL) that
 *             receives the compressed bytes of every chunk.  The stream is 2 bytes of zlib header (78 5E), the chunks
 *             back to back, 03 00 and the adler32; every chunk is a raw deflate block sequence that starts and ends on a
 *             byte boundary and references nothing in front of itself, so a reader that knows these sizes can inflate
 *             the chunks in parallel (the drop-in library stores them as the container's "DZIX" trailer). */
size_t dctzhip_deflate_bound(size_t n);
size_t dctzhip_deflate_chunk_bytes(void);
int dctzhip_deflate(dctzhip_ctx *ctx, int nsec, const void *const *d_src, const size_t *n, void *const *d_dst,
                    const size_t *cap, size_t *out_len, uint32_t *const *chunk_sizes);
/* The same with one flag word per section (NULL: none).  DCTZHIP_DEFLATE_LITERALS: do not search the section for
 * matches -- for bytes of floats (DC, AC_exact), where zlib's own search finds next to nothing; the section is then
 * coded with its byte statistics alone (same size to 0.1 %, a fifth of the parse time). */
#define DCTZHIP_DEFLATE_LITERALS 1u
int dctzhip_deflate_ex(dctzhip_ctx *ctx, int nsec, const void *const *d_src, const size_t *n, void *const *d_dst,
                       const size_t *cap, size_t *out_len, uint32_t *const *chunk_sizes, const unsigned *flags);

/* The reader's side of the same stage: sections written by dctzhip_deflate inflated on the device, one lane per chunk
 * (replaces, for such sections, inflateInit / inflate of dctz-decomp-lib.c:244-322 and the H2D copy of the raw streams).
 *   d_z[i], zlen[i]   the section's zlib stream in device memory
 *   chunk_sizes[i]    host array: compressed bytes of every chunk (the container's "DZIX" index)
 *   raw[i], d_dst[i]  bytes the section inflates to, and where (device)
 *   *ok               1: every chunk decoded, lengths and the adler32 of the content agree with the stream;
 *                     0: something is inconsistent (or the stream is not of this kind) -- the outputs are undefined and
 *                        the caller takes the zlib path, which reports damage the way the reference does.
 * A damaged stream cannot make the kernel read or write outside the buffers described here. */
int dctzhip_inflate(dctzhip_ctx *ctx, int nsec, const void *const *d_z, const size_t *zlen, const uint32_t *const *chunk_sizes,
                    const size_t *raw, void *const *d_dst, int *ok);

/* Diagnostics: element-wise x / divisor computed (a) by the kernels' hoisted-
 * reciprocal division and (b) by the compiler's IEEE division; the two outputs
 * must be bit-identical (tests/test_gpu_parity.py::test_fast_division_is_exact). */
int dctzhip_debug_divide(dctzhip_ctx *ctx, const void *d_x, size_t n, int dtype,
                         double divisor, void *d_fast, void *d_ref);

/* Library/ABI version, "major.minor.patch". */
const char *dctzhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DCTZ_HIP_H */
