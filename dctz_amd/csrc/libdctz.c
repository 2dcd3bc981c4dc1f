/*
 * libdctz.c -- drop-in host library: the reference's public API (include/dctz.h;
 * upstream dctz.h:121-128 and dct.h:17-27) over the MI355X hot path
 * (include/dctz_hip.h).  Plain C, built twice like the reference's Makefile:12-17:
 *   libdctz-ec.so   -DUSE_TRUNCATE
 *   libdctz-qt.so   -DUSE_TRUNCATE -DUSE_QTABLE
 *
 * What runs where
 *   GPU  : calc_data_stat, scaling, block DCT-II/III, binning, QT table, ordered
 *          AC_exact compaction, de-quantisation, de-scaling (dctz-comp-lib.c:186-544,
 *          dctz-decomp-lib.c:358-511) -- every arithmetic step of the hot path.
 *   host : PCIe copies, the zlib tail on 3 pthreads (dctz-comp-lib.c:620-732,
 *          kept as the reference has it) and the 56-byte container header
 *          (dctz.h:96-119; writer dctz-comp-lib.c:775-820, reader
 *          dctz-decomp-lib.c:84-100,186-199).
 * There is no CPU implementation of the GPU stages here: if the HIP library
 * cannot create a context the process exits(1), the reference's own error
 * convention (dctz-comp-lib.c:123-126).
 *
 * Observable behaviour kept from the reference: both entry points return 1;
 * error_bound < 1e-6 prints "ERROR BOUND is not acceptable" and exits(1)
 * (dctz-comp-lib.c:135-138); var->buf is scaled IN PLACE by 1/sf (:193-216);
 * "outSize = ..." / "uncompressed bin_index size is: ..." go to stdout (:841-843,
 * dctz-decomp-lib.c:260-262) unless DCTZ_QUIET is set.  The unconditional dump
 * files ./bin_index.bin and ./AC_exact.bin (:583-595; ./qtable.bin :443-448) are
 * written only when DCTZ_DUMP_STREAMS is set.
 */
#define _GNU_SOURCE
#include "dctz.h"

#include <pthread.h>
#include <sched.h>
#include <unistd.h>
#include "pdeflate.h"
#include <stdint.h>
#include <sys/time.h>

#include "dctz_hip.h"
#include "dctz_container.h"
#include "dctz_fixup_blob.h"
#include "dctz_mask_blob.h"

#ifndef USE_TRUNCATE
#error "build with -DUSE_TRUNCATE (every reference target does, Makefile:13-24)"
#endif

#define DEF_MEM_LEVEL 8 /* dctz-comp-lib.c:25 */

#ifdef USE_QTABLE
#define DCTZ_MODE DCTZHIP_QT
#else
#define DCTZ_MODE DCTZHIP_EC
#endif
#define DCTZ_QT (DCTZ_MODE == DCTZHIP_QT)     /* the variant, as csrc/dctz_container.h takes it */

/* ------------------------------------------------------------------ state -- */
static dctzhip_ctx *g_ctx = NULL;
static struct {
  void *in, *bin, *dc, *ac, *out, *z[3], *idx, *fix;
  size_t in_cap, bin_cap, dc_cap, ac_cap, out_cap, z_cap[3], idx_cap, fix_cap;
} g_dev;
/* Host copies of the raw streams (what the zlib tails read / the inflates write), kept between calls like the device
 * buffers above: a fresh 170 MB allocation per call costs its page faults on the way in and an munmap on the way out
 * (about 25 ms per GiB shard, more than the indexed inflate itself). */
static struct {
  void *p[3];
  size_t cap[3];
} g_host;
static void *host_buf(int i, size_t need) {
  if (need == 0) need = 1;
  if (need > g_host.cap[i]) {
    free(g_host.p[i]);
    g_host.p[i] = malloc(need);
    g_host.cap[i] = g_host.p[i] ? need : 0;
    if (!g_host.p[i]) { fprintf(stderr, "Out of memory: streams\n"); exit(1); }
  }
  return g_host.p[i];
}
static dctz_stage_times g_times;
/* multi-dimensional blocks requested for the next dctz_compress call (dctz.h: dctz_set_block_dims) */
static int g_nd = 0;
static size_t g_dims[3] = {0, 0, 0};

static double now_s(void) {
  struct timeval tv;
  gettimeofday(&tv, NULL);
  return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

static int quiet(void) { return getenv("DCTZ_QUIET") != NULL; }
/* DCTZ_ZLIB_THREADS: unset / <= 3 = the reference's tail (three threads, one single-shot
 * deflate each, dctz-comp-lib.c:620-732).  > 3: chunked deflate on that many threads (pdeflate.c;
 * still one zlib stream per section).  The reader inflates the three sections side by side unless
 * DCTZ_ZLIB_THREADS is 1..3 (then one after the other, dctz-decomp-lib.c:244-322: same bytes out either way).
 * DCTZ_ZLIB_CHUNK: bytes per deflate job (default 256 KiB).  DCTZ_ZLIB_LEVEL: 1..9 for the chunked tail
 * only (default: zlib's default level, as the reference; a lower level trades ratio for host time). */
static int zlib_threads(void) { const char *e = getenv("DCTZ_ZLIB_THREADS"); return e ? atoi(e) : 0; }
/* DCTZ_ZLIB_GPU=1: the entropy stage runs on the device too (include/dctz_hip.h: dctzhip_deflate):
 * the three sections are deflated where k_compress left them and only compressed bytes come back over PCIe.  One zlib
 * stream per section as before (any inflate reads it, dctz-decomp-lib.c:244-322); the bytes -- and the sizes, by a per
 * cent or so -- differ from zlib's, which is why the reference's tail stays the default. */
static int zlib_gpu(void) { const char *e = getenv("DCTZ_ZLIB_GPU"); return e && atoi(e) != 0; }
/* DCTZ_FAST_MEAN=1: header.mean = the tree-order sum / N that the compress kernels produce anyway, instead of the
 * reference's serial-order sum (util.c:18-28).  The field is written but never read back (dctz-decomp-lib.c:499 is
 * commented out); the serial chain of N dependent additions is what bounds a call once the entropy stage is on the GPU
 * (50 ms per GiB on one host core).  Off by default: the header is then bit-identical to the reference's. */
static int fast_mean(void) { const char *e = getenv("DCTZ_FAST_MEAN"); return e && atoi(e) != 0; }
/* DCTZ_SCALE_HOST: 1 = x / sf is written into the caller's buffer by host threads, 0 = by the GPU + a D2H copy.
 * Default: host threads exactly when the entropy stage runs on the GPU (the host cores are idle then). */
static int scale_on_host(int gpu_tail) { const char *e = getenv("DCTZ_SCALE_HOST"); return e ? atoi(e) != 0 : gpu_tail; }
static size_t zlib_chunk(void) {
  const char *e = getenv("DCTZ_ZLIB_CHUNK");
  long long v = e ? atoll(e) : 0;
  return v >= 32768 ? (size_t)v : (size_t)262144;
}

static void die(const char *what) {
  fprintf(stderr, "libdctz: %s: %s\n", what, dctzhip_last_error(g_ctx));
  exit(1);
}

/* Which GPU: DCTZ_DEVICE (an index), else the process's rank on its node -- DCTZ_RANK, or what the usual launchers export
 * (LOCAL_RANK, OMPI_COMM_WORLD_LOCAL_RANK, SLURM_LOCALID) -- modulo the GPUs visible: one process per GPU, every process
 * compresses its own shards (they are independent dctz_compress calls), see INTEGRATION.md section D. */
static int pick_device(void) {
  const char *d = getenv("DCTZ_DEVICE");
  if (d) return atoi(d);
  const char *names[] = {"DCTZ_RANK", "LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "SLURM_LOCALID"};
  for (int i = 0; i < 4; i++) {
    const char *r = getenv(names[i]);
    if (r && *r) { const int n = dctzhip_device_count(); return n > 0 ? atoi(r) % n : -1; }
  }
  return -1;                                   /* the current HIP device */
}

static dctzhip_ctx *ctx(void) {
  if (!g_ctx) {
    if (dctzhip_ctx_create(&g_ctx, pick_device()) != DCTZHIP_OK) {
      fprintf(stderr, "libdctz: no usable MI355X context: %s\n", dctzhip_last_error(NULL));
      exit(1);
    }
  }
  return g_ctx;
}

static void grow(void **p, size_t *cap, size_t need) {
  if (need <= *cap) return;
  if (*p && dctzhip_free(ctx(), *p) != DCTZHIP_OK) die("dctzhip_free");
  *p = NULL;
  *cap = 0;
  if (dctzhip_malloc(ctx(), p, need) != DCTZHIP_OK) die("Out of memory (device)");
  *cap = need;
}

void dctz_last_stage_times(dctz_stage_times *t) { if (t) *t = g_times; }

/* ------------------------------------------------------------- zlib tail --- */
/* One deflate stream per thread, finished in one call; the compressed size is
 * the thread's exit value (dctz-comp-lib.c:75-88). */
void *compress_thread(void *arg) {
  z_stream *zs = (z_stream *)arg;
  deflate(zs, Z_FINISH);
  uLong produced = zs->total_out;
  deflateEnd(zs);
  pthread_exit((void *)produced);
}

/* Our own section jobs feed zlib in pieces of at most 1 GiB: avail_in / avail_out are 32-bit (uInt), and a section can
 * be larger (AC_exact: 4 bytes x up to 2^31 - 1 exceptions).  Same stream as one deflate(Z_FINISH) call of the whole. */
static size_t z_piece(void) {                /* DCTZ_ZLIB_PIECE: test hook (tiny pieces exercise the refill loops) */
  static size_t v = 0;
  if (!v) { const char *e = getenv("DCTZ_ZLIB_PIECE"); long long x = e ? atoll(e) : 0; v = (x >= 64 && x <= (1ll << 30)) ? (size_t)x : ((size_t)1 << 30); }
  return v;
}
#define Z_PIECE z_piece()
typedef struct {
  z_stream zs;
  pthread_t th;
  Bytef *dst;
  uLong bound;
  const Bytef *src;
  size_t left;
  int rc;
} zjob;

static void *zjob_main(void *arg) {
  zjob *j = (zjob *)arg;
  z_stream *zs = &j->zs;
  size_t out_left = j->bound;
  zs->next_in = (Bytef *)j->src; zs->avail_in = 0;
  zs->next_out = j->dst; zs->avail_out = 0;
  for (;;) {
    if (zs->avail_in == 0 && j->left) {
      const size_t piece = j->left < Z_PIECE ? j->left : Z_PIECE;
      zs->avail_in = (uInt)piece; j->left -= piece;                /* next_in already points behind the previous piece */
    }
    if (zs->avail_out == 0 && out_left) {
      const size_t piece = out_left < Z_PIECE ? out_left : Z_PIECE;
      zs->avail_out = (uInt)piece; out_left -= piece;
    }
    const int rc = deflate(zs, j->left ? Z_NO_FLUSH : Z_FINISH);
    if (rc == Z_STREAM_END) break;
    if (rc != Z_OK && !(rc == Z_BUF_ERROR && (zs->avail_in == 0 || zs->avail_out == 0) && (j->left || out_left))) { j->rc = rc ? rc : -1; break; }
  }
  uLong produced = zs->total_out;
  deflateEnd(zs);
  return (void *)produced;
}

static void zjob_start(zjob *j, const void *src, size_t nbytes, pthread_attr_t *attr) {
  j->bound = (nbytes <= 0xffffffffu) ? compressBound((uLong)nbytes) : (uLong)(nbytes + nbytes / 1000 + (nbytes >> 25) * 16 + 4096);
  j->dst = (Bytef *)malloc(j->bound ? j->bound : 1);
  if (!j->dst) { fprintf(stderr, "Out of memory: zlib buffer\n"); exit(1); }
  memset(&j->zs, 0, sizeof(j->zs));
  j->zs.zalloc = Z_NULL; j->zs.zfree = Z_NULL; j->zs.opaque = Z_NULL;
  /* dctz-comp-lib.c:642-643: default level, 32K window, memLevel 8, default strategy */
  deflateInit2(&j->zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15, DEF_MEM_LEVEL, Z_DEFAULT_STRATEGY);
  j->zs.data_type = Z_UNKNOWN;
  j->src = (const Bytef *)src; j->left = nbytes; j->rc = 0;
  if (pthread_create(&j->th, attr, zjob_main, j)) {
    fprintf(stderr, "Error creating thread\n");
    exit(0); /* dctz-comp-lib.c:651-654 */
  }
}

static uLong zjob_join(zjob *j) {
  void *ret = NULL;
  pthread_join(j->th, &ret);
  if (j->rc) { fprintf(stderr, "libdctz: deflate failed (%d)\n", j->rc); exit(1); }
  return (uLong)ret;
}

static uLong inflate_into(const Bytef *src, uLong src_len, void *dst, size_t dst_len) {
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  zs.zalloc = Z_NULL; zs.zfree = Z_NULL; zs.opaque = Z_NULL;
  inflateInit(&zs); /* dctz-decomp-lib.c:250 */
  zs.avail_in = (uInt)src_len;                                       /* a section's compressed size is a uint32 of the header */
  zs.next_in = (Bytef *)src;
  zs.next_out = (Bytef *)dst;
  size_t out_left = dst_len;
  for (;;) {                                                         /* the inflated size may exceed 4 GiB */
    if (zs.avail_out == 0 && out_left) {
      const size_t piece = out_left < Z_PIECE ? out_left : Z_PIECE;
      zs.avail_out = (uInt)piece; out_left -= piece;
    }
    const int rc = inflate(&zs, Z_NO_FLUSH);
    if (rc != Z_OK || (zs.avail_out != 0) || !out_left) break;
  }
  uLong produced = zs.total_out;
  inflateEnd(&zs);
  return produced;
}

/* The header's `mean` in the reference's own summation order (util.c:18-28 / :31-41: x[1] + x[2] + ...
 * one after the other, in the data type).  That chain of roundings is inherently sequential:
 * one GPU lane needs ~30 ns per dependent add (k_serial_sum: 4 s per GiB, fine underneath the
 * reference's 7 s zlib tail), a host core ~1 ns.  With the chunked tail the zlib stage is too
 * short to hide the GPU version, so the sum runs on one host thread over the caller's array,
 * which is where the reference computes it too; it must finish before x/sf is copied back. */
#define MEAN_BLOCK ((size_t)1 << 20)          /* elements between two progress reports of the serial sum */
typedef struct {
  const void *x;
  size_t n;
  int is_d;
  double mean;
  size_t progress;              /* elements the sum has consumed (released block by block: the in-place scaling follows behind) */
} host_mean_job;
static void *host_mean_main(void *arg) {
  host_mean_job *j = (host_mean_job *)arg;
  if (j->is_d) {
    const double *x = (const double *)j->x;
    double sum = 0.0;
    for (size_t b = 1; b < j->n; b += MEAN_BLOCK) {
      const size_t e = b + MEAN_BLOCK < j->n ? b + MEAN_BLOCK : j->n;
      for (size_t i = b; i < e; i++) sum += x[i];           /* util.c:22: starts at i = 1 */
      __atomic_store_n(&j->progress, e, __ATOMIC_RELEASE);
    }
    j->mean = sum / (double)(int)j->n;
  } else {
    const float *x = (const float *)j->x;
    float sum = 0.0f;
    for (size_t b = 1; b < j->n; b += MEAN_BLOCK) {
      const size_t e = b + MEAN_BLOCK < j->n ? b + MEAN_BLOCK : j->n;
      for (size_t i = b; i < e; i++) sum += x[i];           /* util.c:35 */
      __atomic_store_n(&j->progress, e, __ATOMIC_RELEASE);
    }
    j->mean = (double)(sum / (float)(int)j->n);
  }
  __atomic_store_n(&j->progress, j->n, __ATOMIC_RELEASE);
  return NULL;
}

/* The reference's in-place "/= sf" (dctz-comp-lib.c:193-216) on host threads, for the device entropy stage: there the
 * tail is too short to hide a 1 GiB write-back over PCIe, and the host cores are idle.  Same operation as the
 * reference's loop (IEEE division in the data type), so the caller's buffer ends up bit-identical to x / sf.  An
 * element may only change once the serial-order mean has read it: the workers take 1 Mi-element blocks in order and
 * follow the sum's progress counter, so the scaling ends a block after the sum does instead of starting there. */
typedef struct {
  void *x;
  size_t n;
  int is_d, threads;
  double sf;
  pthread_t *wait_for;          /* the serial-mean thread (joined here), or NULL */
  host_mean_job *mean;          /* its progress: elements it has read for good, or NULL = all */
  size_t next;                  /* next block to scale (workers take blocks in order) */
} scale_mgr;
static void *scale_worker(void *arg) {
  scale_mgr *m = (scale_mgr *)arg;
  for (;;) {
    const size_t lo = __atomic_fetch_add(&m->next, MEAN_BLOCK, __ATOMIC_RELAXED);
    if (lo >= m->n) break;
    const size_t hi = lo + MEAN_BLOCK < m->n ? lo + MEAN_BLOCK : m->n;
    while (m->mean && __atomic_load_n(&m->mean->progress, __ATOMIC_ACQUIRE) < hi) sched_yield();   /* the sum still needs the originals */
    if (m->is_d) { double *x = (double *)m->x; const double sf = m->sf; for (size_t i = lo; i < hi; i++) x[i] /= sf; }
    else { float *x = (float *)m->x; const float sf = (float)m->sf; for (size_t i = lo; i < hi; i++) x[i] /= sf; }
  }
  return NULL;
}
static void *scale_mgr_main(void *arg) {
  scale_mgr *m = (scale_mgr *)arg;
  int T = m->threads < 1 ? 1 : (m->threads > 64 ? 64 : m->threads);
  if ((size_t)T > m->n / MEAN_BLOCK + 1) T = (int)(m->n / MEAN_BLOCK + 1);
  if (m->mean && T > 6) T = 6;              /* behind the serial sum (one block per ~0.5 ms) a few workers keep up; more would only spin */
  pthread_t th[64];
  int started = 0;
  for (int t = 1; t < T; t++) { if (pthread_create(&th[started], NULL, scale_worker, m) == 0) started++; }
  scale_worker(m);
  for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
  if (m->wait_for) pthread_join(*m->wait_for, NULL);
  return NULL;
}
static int host_threads(void) {
  int t = zlib_threads();
  if (t <= 0) { long nc = sysconf(_SC_NPROCESSORS_ONLN); t = nc > 32 ? 32 : (nc < 1 ? 1 : (int)nc); }
  return t;
}

typedef struct {
  dctz_pd_section sec[3];
  int threads, rc;
  size_t chunk;
} pd_args;
static void *pd_main(void *arg) {
  pd_args *a = (pd_args *)arg;
  a->rc = dctz_pdeflate_many(a->sec, 3, a->threads, a->chunk);
  return NULL;
}

typedef struct {
  const Bytef *src;
  uLong src_len, dst_len, produced;
  void *dst;
} inflate_job;
static void *inflate_main(void *arg) {
  inflate_job *j = (inflate_job *)arg;
  j->produced = inflate_into(j->src, j->src_len, j->dst, j->dst_len);
  return NULL;
}

static void put_be32(unsigned char *p, uLong v) { p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v; }
static uLong get_be32(const unsigned char *p) { return ((uLong)p[0] << 24) | ((uLong)p[1] << 16) | ((uLong)p[2] << 8) | (uLong)p[3]; }
/* ---- sections whose deflate blocks are independent chunks ("DZIX" trailer, dctz.h): inflated side by side ---- */
typedef struct {
  const unsigned char *src;   /* chunk bytes (raw deflate, byte aligned) */
  unsigned int zlen;
  unsigned char *dst;
  unsigned int len;           /* bytes the chunk must inflate to */
  uLong adler;
  int err;
} ix_chunk;
typedef struct {
  ix_chunk *chunks;
  size_t nchunks, next;
  pthread_mutex_t mu;
} ix_queue;
static void *ix_worker(void *arg) {
  ix_queue *q = (ix_queue *)arg;
  for (;;) {
    pthread_mutex_lock(&q->mu);
    size_t lo = q->next, hi = lo + 16 < q->nchunks ? lo + 16 : q->nchunks;   /* a few chunks per visit to the counter */
    q->next = hi;
    pthread_mutex_unlock(&q->mu);
    if (lo >= hi) break;
    for (size_t i = lo; i < hi; i++) {
      ix_chunk *c = &q->chunks[i];
      z_stream zs;
      memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) { c->err = 1; continue; }
      zs.next_in = (Bytef *)c->src; zs.avail_in = c->zlen;
      zs.next_out = c->dst; zs.avail_out = c->len;
      const int rc = inflate(&zs, Z_SYNC_FLUSH);
      if ((rc != Z_OK && rc != Z_BUF_ERROR) || zs.avail_in != 0 || zs.avail_out != 0) {
        c->err = 1;
        memset(zs.next_out, 0, zs.avail_out);   /* what a damaged chunk did not write: zeros, not what the buffer held before */
      }
      inflateEnd(&zs);
      c->adler = adler32(adler32(0L, Z_NULL, 0), c->dst, c->len);
    }
  }
  return NULL;
}
/* Inflates a list of independent chunks side by side on DCTZ_ZLIB_THREADS host threads (default: the cores, at most 32). */
static void ix_run(ix_chunk *chunks, size_t total) {
  int threads = zlib_threads();
  if (threads <= 0) { long nc = sysconf(_SC_NPROCESSORS_ONLN); threads = nc > 32 ? 32 : (nc < 1 ? 1 : (int)nc); }
  if ((size_t)threads > total) threads = total ? (int)total : 1;
  ix_queue q;
  q.chunks = chunks; q.nchunks = total; q.next = 0;
  pthread_mutex_init(&q.mu, NULL);
  pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)threads);
  int started = 0;
  if (th) for (int t = 0; t < threads - 1; t++) { if (pthread_create(&th[started], NULL, ix_worker, &q)) break; started++; }
  ix_worker(&q);
  for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
  free(th);
  pthread_mutex_destroy(&q.mu);
}

/* The three sections of an indexed container inflated chunk by chunk on host threads (sizes / chunk from dzc_read_index).
 * Returns 1, or 0 when a chunk does not inflate or the content's adler32 is not the stream's: the caller then hands the
 * sections to the ordinary inflate, which treats damage the way the reference's reader does (dctz-decomp-lib.c:244-322
 * ignores inflate's return code). */
static int inflate_indexed(const dzc_view *v, unsigned char *const dst[3], size_t chunk, uint32_t *const sizes[3]) {
  const unsigned char *const *sec = v->sec;
  const unsigned int *zlen = v->zlen;
  const size_t *raw = v->raw;
  size_t nch[3], total = 0;
  for (int i = 0; i < 3; i++) { nch[i] = (raw[i] + chunk - 1) / chunk; total += nch[i]; }
  ix_chunk *chunks = (ix_chunk *)calloc(total ? total : 1, sizeof(ix_chunk));
  if (!chunks) { fprintf(stderr, "Out of memory: chunk list\n"); exit(1); }
  size_t k = 0;
  for (int i = 0; i < 3; i++) {
    size_t off = 2;
    for (size_t j = 0; j < nch[i]; j++, k++) {
      chunks[k].src = sec[i] + off; chunks[k].zlen = sizes[i][j];
      chunks[k].dst = dst[i] + j * chunk;
      chunks[k].len = (unsigned int)(raw[i] - j * chunk < chunk ? raw[i] - j * chunk : chunk);
      off += sizes[i][j];
    }
  }
  ix_run(chunks, total);
  int ok = 1;
  k = 0;
  for (int i = 0; i < 3 && ok; i++) {                   /* what inflate() checks at the end of a stream: the adler32 of the content */
    uLong a = adler32(0L, Z_NULL, 0);
    for (size_t j = 0; j < nch[i]; j++, k++) { if (chunks[k].err) ok = 0; a = adler32_combine(a, chunks[k].adler, (z_off_t)chunks[k].len); }
    if (a != get_be32(sec[i] + zlen[i] - 4)) ok = 0;
  }
  free(chunks);
  if (!ok) fprintf(stderr, "libdctz: a chunk of an indexed section does not inflate; falling back to the one-stream inflate\n");
  return ok;
}

/* DCTZ_INFLATE_GPU=1: indexed sections are inflated on the device (one lane per chunk) instead of by host threads.
 * Off by default: a lane decodes its 16 KiB alone, which takes 18 - 30 ms per section however few chunks there are
 * (38 ms for the three sections of a 1 GiB shard side by side), where sixteen host threads need 19 ms; it pays on hosts with few
 * cores (the work is 0.5 core-seconds per GiB) and takes the raw streams off PCIe. */
static int inflate_gpu(void) { const char *e = getenv("DCTZ_INFLATE_GPU"); return e && atoi(e) != 0; }

static void dump_file(const char *name, const void *p, size_t bytes) {
  FILE *fp = fopen(name, "wb");
  if (!fp) return;
  fwrite(p, bytes, 1, fp);
  fclose(fp);
}

/* ------------------------------------------------- multi-dimensional blocks --- */
int dctz_set_block_dims(int ndims, const size_t *dims) {
  g_nd = 0;
  if (ndims <= 1) return 0;
  if (ndims > 3 || !dims) return -1;
  for (int i = 0; i < ndims; i++) if (dims[i] == 0 || dims[i] > 0x7FFFFFFFu) return -1;
  for (int i = 0; i < 3; i++) g_dims[i] = i < ndims ? dims[i] : 1;
  g_nd = ndims;
  return 0;
}

/* geometry of this call: the explicit request (one call only), else DCTZ_BLOCK_DIMS when its product is N */
static int take_block_dims(size_t n, size_t dims[3]) {
  int nd = g_nd;
  if (nd) { for (int i = 0; i < 3; i++) dims[i] = g_dims[i]; g_nd = 0; }
  else {
    const char *e = getenv("DCTZ_BLOCK_DIMS");
    if (!e || !*e) return 0;
    char *end = NULL;
    while (nd < 3) {
      const unsigned long long v = strtoull(e, &end, 10);
      if (end == e || v == 0 || v > 0x7FFFFFFFull) return 0;
      dims[nd++] = (size_t)v;
      if (*end != 'x' && *end != 'X') break;
      e = end + 1;
    }
    if (*end != 0 || nd < 2) return 0;
  }
  size_t prod = 1;
  for (int i = 0; i < nd; i++) prod *= dims[i];
  if (prod != n) {
    if (nd && !getenv("DCTZ_BLOCK_DIMS")) { fprintf(stderr, "libdctz: block dims do not multiply to N\n"); exit(1); }
    return 0;                                    /* the environment describes some other array of the run */
  }
  return nd;
}

/* ---- dctz_compress of a large array, pipelined (round 4) --------------------------------------------------------------
 * With the entropy stage on the device a 1 GiB call was H2D 19.4 ms -> kernels 0.3 -> deflate 2.6 -> D2H of the
 * compressed sections 4.5, one after the other, the host cores scaling the caller's array meanwhile: 27 ms, of which the
 * GPU worked for three.  The blocks of an array are independent once its scaling factor is known (util.c:29: a function of
 * max|x| alone), so:
 *   * the array crosses PCIe in GROUPS of DCTZ_PIPE_GROUP elements (default 8 Mi; dctzhip_h2d_pipe_*);
 *   * host threads take max|x| / min|x| of the caller's array while the first groups are under way (3 ms);
 *   * every group that has landed is compressed with the ARRAY's statistics (dctzhip_compress_part: same streams as the
 *     one call, AC_exact appended behind the groups in front), its bin_index and DC are deflated on the device -- the
 *     entropy stage codes 16 KiB chunks that reference nothing outside themselves, and a group is a whole number of chunks
 *     of both sections, so the groups' pieces concatenate to exactly the stream of the one call (adler32_combine for the
 *     check value) -- and the compressed bytes go back while the next groups are still arriving;
 *   * the in-place x /= sf of the caller's array (dctz-comp-lib.c:193-216) follows the copy: a block is divided once the
 *     group it lies in is on the device;
 *   * behind the last group only AC_exact (known in full only then) is left to deflate and bring back.
 * Same container as the serial path of this mode except for the header's `mean` (a tree-order sum either way; this path
 * adds the groups' sums).  DCTZ_PIPELINE=0: the serial path. */
static int pipeline_on(void) { const char *e = getenv("DCTZ_PIPELINE"); return e ? atoi(e) != 0 : 1; }
static size_t pipe_group(void) {
  const char *e = getenv("DCTZ_PIPE_GROUP");
  long long v = e ? atoll(e) : 0;
  return v >= (1 << 18) ? ((size_t)v & ~(size_t)((1 << 18) - 1)) : ((size_t)1 << 23);   /* a multiple of 256 Ki elements */
}
typedef struct { const void *x; size_t lo, hi; int is_d; double mx, mn; } mm_job;
/* util.c:18-25: max|x| and min|x|.  A NaN never wins a comparison there; vmaxpd / vminpd return their SECOND operand when
 * the comparison is unordered, so with the running value second a NaN element is passed over the same way. */
__attribute__((target("avx2"))) static void mm_range_avx2(mm_job *j) {
  if (j->is_d) {
    typedef double v4 __attribute__((vector_size(32), aligned(8)));
    typedef long long m4 __attribute__((vector_size(32)));
    const double *x = (const double *)j->x;
    const m4 absm = {0x7fffffffffffffffLL, 0x7fffffffffffffffLL, 0x7fffffffffffffffLL, 0x7fffffffffffffffLL};
    v4 mx[4], mn[4];
    for (int u = 0; u < 4; u++) { mx[u] = (v4){-1.0, -1.0, -1.0, -1.0}; mn[u] = (v4){INFINITY, INFINITY, INFINITY, INFINITY}; }
    size_t i = j->lo;
    for (; i + 16 <= j->hi; i += 16)
      for (int u = 0; u < 4; u++) {
        const v4 a = (v4)((m4)(*(const v4 *)(x + i + 4 * u)) & absm);
        mx[u] = __builtin_ia32_maxpd256(a, mx[u]);
        mn[u] = __builtin_ia32_minpd256(a, mn[u]);
      }
    double m = -1.0, l = INFINITY;
    for (int u = 0; u < 4; u++) for (int k = 0; k < 4; k++) { if (mx[u][k] > m) m = mx[u][k]; if (mn[u][k] < l) l = mn[u][k]; }
    for (; i < j->hi; i++) { const double a = fabs(x[i]); if (a > m) m = a; if (a < l) l = a; }
    j->mx = m; j->mn = l;
  } else {
    typedef float v8 __attribute__((vector_size(32), aligned(4)));
    typedef int m8 __attribute__((vector_size(32)));
    const float *x = (const float *)j->x;
    const m8 absm = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    v8 mx[4], mn[4];
    for (int u = 0; u < 4; u++) for (int k = 0; k < 8; k++) { mx[u][k] = -1.0f; mn[u][k] = INFINITY; }
    size_t i = j->lo;
    for (; i + 32 <= j->hi; i += 32)
      for (int u = 0; u < 4; u++) {
        const v8 a = (v8)((m8)(*(const v8 *)(x + i + 8 * u)) & absm);
        mx[u] = __builtin_ia32_maxps256(a, mx[u]);
        mn[u] = __builtin_ia32_minps256(a, mn[u]);
      }
    float m = -1.0f, l = INFINITY;
    for (int u = 0; u < 4; u++) for (int k = 0; k < 8; k++) { if (mx[u][k] > m) m = mx[u][k]; if (mn[u][k] < l) l = mn[u][k]; }
    for (; i < j->hi; i++) { const float a = fabsf(x[i]); if (a > m) m = a; if (a < l) l = a; }
    j->mx = (double)m; j->mn = (double)l;
  }
}
static void *mm_main(void *arg) {
  mm_job *j = (mm_job *)arg;
  if (__builtin_cpu_supports("avx2")) { mm_range_avx2(j); return NULL; }
  enum { U = 8 };                               /* independent chains: a single running maximum is one element per 4 cycles */
  if (j->is_d) {
    const double *x = (const double *)j->x;
    double mx[U], mn[U];
    for (int u = 0; u < U; u++) { mx[u] = -1.0; mn[u] = INFINITY; }
    size_t i = j->lo;
    for (; i + U <= j->hi; i += U)
      for (int u = 0; u < U; u++) { const double a = fabs(x[i + u]); if (a > mx[u]) mx[u] = a; if (a < mn[u]) mn[u] = a; }
    for (; i < j->hi; i++) { const double a = fabs(x[i]); if (a > mx[0]) mx[0] = a; if (a < mn[0]) mn[0] = a; }
    for (int u = 1; u < U; u++) { if (mx[u] > mx[0]) mx[0] = mx[u]; if (mn[u] < mn[0]) mn[0] = mn[u]; }
    j->mx = mx[0]; j->mn = mn[0];
  } else {
    const float *x = (const float *)j->x;
    float mx[U], mn[U];
    for (int u = 0; u < U; u++) { mx[u] = -1.0f; mn[u] = INFINITY; }
    size_t i = j->lo;
    for (; i + U <= j->hi; i += U)
      for (int u = 0; u < U; u++) { const float a = fabsf(x[i + u]); if (a > mx[u]) mx[u] = a; if (a < mn[u]) mn[u] = a; }
    for (; i < j->hi; i++) { const float a = fabsf(x[i]); if (a > mx[0]) mx[0] = a; if (a < mn[0]) mn[0] = a; }
    for (int u = 1; u < U; u++) { if (mx[u] > mx[0]) mx[0] = mx[u]; if (mn[u] < mn[0]) mn[0] = mn[u]; }
    j->mx = (double)mx[0]; j->mn = (double)mn[0];
  }
  return NULL;
}
/* x[lo, hi) /= sf, the reference's loop (IEEE division in the data type); four / eight lanes at a time where the CPU has
 * AVX2 (vdivpd / vdivps round like divsd / divss) */
__attribute__((target("avx2"))) static void scale_range_avx2(void *xv, size_t lo, size_t hi, int is_d, double sf) {
  if (is_d) {
    double *x = (double *)xv;
    typedef double v4 __attribute__((vector_size(32), aligned(8)));
    const v4 d = {sf, sf, sf, sf};
    size_t i = lo;
    for (; i + 4 <= hi; i += 4) { v4 v = *(v4 *)(x + i); v = v / d; *(v4 *)(x + i) = v; }
    for (; i < hi; i++) x[i] /= sf;
  } else {
    float *x = (float *)xv;
    const float f = (float)sf;
    typedef float v8 __attribute__((vector_size(32), aligned(4)));
    const v8 d = {f, f, f, f, f, f, f, f};
    size_t i = lo;
    for (; i + 8 <= hi; i += 8) { v8 v = *(v8 *)(x + i); v = v / d; *(v8 *)(x + i) = v; }
    for (; i < hi; i++) x[i] /= f;
  }
}
static void scale_range(void *xv, size_t lo, size_t hi, int is_d, double sf) {
  if (__builtin_cpu_supports("avx2")) { scale_range_avx2(xv, lo, hi, is_d, sf); return; }
  if (is_d) { double *x = (double *)xv; for (size_t i = lo; i < hi; i++) x[i] /= sf; }
  else { float *x = (float *)xv; const float f = (float)sf; for (size_t i = lo; i < hi; i++) x[i] /= f; }
}
#define FOLLOW_BLOCK ((size_t)1 << 17)        /* elements a worker of the follower divides at a time */
typedef struct {
  void *x; size_t n; int is_d; double sf;
  size_t landed;                /* elements of the caller's array the copy has finished with (released group by group) */
  size_t next;
  int failed;
} follow_job;
static void *follow_worker(void *arg) {
  follow_job *f = (follow_job *)arg;
  for (;;) {
    const size_t lo = __atomic_fetch_add(&f->next, FOLLOW_BLOCK, __ATOMIC_RELAXED);
    if (lo >= f->n) break;
    const size_t hi = lo + FOLLOW_BLOCK < f->n ? lo + FOLLOW_BLOCK : f->n;
    while (__atomic_load_n(&f->landed, __ATOMIC_ACQUIRE) < hi) {
      if (__atomic_load_n(&f->failed, __ATOMIC_ACQUIRE)) return NULL;
      usleep(20);
    }
    scale_range(f->x, lo, hi, f->is_d, f->sf);
  }
  return NULL;
}
typedef struct { dctzhip_ctx *c; follow_job *f; size_t gel, ts; } track_job;
static void *track_main(void *arg) {            /* releases the groups to the follower as their copies complete */
  track_job *t = (track_job *)arg;
  for (size_t e = 0; e < t->f->n;) {
    e = e + t->gel < t->f->n ? e + t->gel : t->f->n;
    if (dctzhip_h2d_pipe_landed(t->c, e * t->ts) != DCTZHIP_OK) { __atomic_store_n(&t->f->failed, 1, __ATOMIC_RELEASE); return NULL; }
    __atomic_store_n(&t->f->landed, e, __ATOMIC_RELEASE);
  }
  return NULL;
}
/* the drainer: compressed pieces of finished groups, device -> host, in order, beside the calling thread */
typedef struct {
  const unsigned char *src;     /* device: a piece's stream (78 5E | chunks | 03 00 | adler32) */
  size_t len, raw;              /* its length; the bytes it inflates to */
  int sec;
} drain_piece;
typedef struct {
  dctzhip_ctx *c;
  drain_piece *q;
  size_t posted, cap;           /* pieces posted so far (released by the calling thread) */
  size_t done;                  /* pieces brought back so far (released by the drainer) */
  int closed, failed;
  unsigned char *base[3];       /* where a section's stream is assembled on the host */
  size_t off[3];                /* its bytes so far, trailer excluded */
  uLong adler[3];
  int started[3];
} drain_job;
static void *drain_main(void *arg) {
  drain_job *d = (drain_job *)arg;
  for (size_t k = 0;; k++) {
    while (__atomic_load_n(&d->posted, __ATOMIC_ACQUIRE) <= k) {
      if (__atomic_load_n(&d->closed, __ATOMIC_ACQUIRE) && __atomic_load_n(&d->posted, __ATOMIC_ACQUIRE) <= k) return NULL;
      usleep(10);
    }
    const drain_piece *p = &d->q[k];
    /* the first piece of a section keeps its two header bytes; every piece's trailer is overwritten by the next piece's chunks */
    const size_t skip = d->started[p->sec] ? 2 : 0;
    unsigned char *at = d->base[p->sec] + d->off[p->sec];
    if (p->len < 8 || dctzhip_memcpy_d2h_side(d->c, at, p->src + skip, p->len - skip) != DCTZHIP_OK) { __atomic_store_n(&d->failed, 1, __ATOMIC_RELEASE); return NULL; }
    d->off[p->sec] += p->len - skip - 6;
    const uLong a = get_be32(d->base[p->sec] + d->off[p->sec] + 2);
    d->adler[p->sec] = d->started[p->sec] ? adler32_combine(d->adler[p->sec], a, (z_off_t)p->raw) : a;
    d->started[p->sec] = 1;
    __atomic_store_n(&d->done, k + 1, __ATOMIC_RELEASE);
  }
}
typedef struct { unsigned char *dst; const unsigned char *src; size_t n; } pcopy_job;
static void *pcopy_main(void *arg) { pcopy_job *j = (pcopy_job *)arg; memcpy(j->dst, j->src, j->n); return NULL; }
static void par_memcpy(void *dst, const void *src, size_t n, int T) {
  if (T > 16) T = 16;
  if (n < ((size_t)1 << 20) || T < 2) { memcpy(dst, src, n); return; }
  pcopy_job j[16];
  pthread_t th[16];
  int started = 0;
  const size_t per = (n / (size_t)T + 4095) & ~(size_t)4095;
  for (int t = 0; t < T; t++) {
    const size_t lo = per * (size_t)t;
    if (lo >= n) break;
    j[t].dst = (unsigned char *)dst + lo; j[t].src = (const unsigned char *)src + lo; j[t].n = n - lo < per ? n - lo : per;
    if (t && pthread_create(&th[started], NULL, pcopy_main, &j[t]) == 0) started++; else pcopy_main(&j[t]);
  }
  for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
}
/* returns 1: the container is written; 0: not applicable, the caller takes the serial path */
static int compress_pipelined(dctzhip_ctx *c, t_var *var, void *host_in, size_t n, int is_d, double error_bound, t_var *var_z, size_t *outSize,
                              double t_begin) {
  if (DCTZ_MODE != DCTZHIP_EC) return 0;          /* QT: the table is a property of the whole array (dctz-comp-lib.c:435-476) */
  const size_t ts = is_d ? sizeof(double) : sizeof(float);
  const int dtype = is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const size_t chunk = dctzhip_deflate_chunk_bytes();
  /* groups of 16 Mi elements unless DCTZ_PIPE_GROUP says otherwise: a group's entropy stage is a millisecond whatever the
   * group's size (four latency-bound kernels per section), a 128 MiB group takes 2.4 ms to arrive */
  const size_t gel = getenv("DCTZ_PIPE_GROUP") ? pipe_group() : ((size_t)1 << 24);
  if (gel % (16 * chunk) != 0 || n < 4 * gel) return 0;
  if (is_d ? isnan(((const double *)host_in)[0]) : isnan(((const float *)host_in)[0])) return 0;   /* util.c:18-19: max = NaN from the start */
  const size_t G = (n + gel - 1) / gel, nblk = CEIL(n, BLK_SZ);
  if (G > DCTZHIP_H2D_PIPE_MAX_GROUPS) return 0;         /* (a small DCTZ_PIPE_GROUP on a large array: more groups than a pipe holds -> the serial path) */
  const int dbg = getenv("DCTZ_PIPE_DEBUG") != NULL;
  /* the first element of every group, as the caller gave it (the follower divides the array while the groups' sums come in) */
  double *firsts = (double *)malloc(G * sizeof(double));
  if (!firsts) { fprintf(stderr, "Out of memory\n"); exit(1); }
  for (size_t g = 0; g < G; g++) firsts[g] = is_d ? ((const double *)host_in)[g * gel] : (double)((const float *)host_in)[g * gel];

  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.bin, &g_dev.bin_cap, n);
  grow(&g_dev.dc, &g_dev.dc_cap, nblk * sizeof(float));
  grow(&g_dev.ac, &g_dev.ac_cap, n * sizeof(float));
  /* every group's pieces have slots of their own in the device buffers of the compressed sections (the drainer is still
   * reading a group's while the next group's are written); AC_exact: what a group can add, plus the chunk carried over */
  const size_t bound[3] = {(dctzhip_deflate_bound(gel) + 255) & ~(size_t)255, (dctzhip_deflate_bound(gel / 16) + 255) & ~(size_t)255,
                           (dctzhip_deflate_bound(gel * sizeof(float) + chunk) + 255) & ~(size_t)255};
  for (int i = 0; i < 3; i++) grow(&g_dev.z[i], &g_dev.z_cap[i], G * bound[i]);
  const size_t bpg = gel / chunk, dpg = gel / 16 / chunk;       /* chunks of bin_index / DC per group */
  size_t ix_n[3] = {(n + chunk - 1) / chunk, (nblk * sizeof(float) + chunk - 1) / chunk, 0};
  uint32_t *ix[3] = {(uint32_t *)malloc((ix_n[0] + 1) * sizeof(uint32_t)), (uint32_t *)malloc((ix_n[1] + 1) * sizeof(uint32_t)),
                     (uint32_t *)malloc((n * sizeof(float) / chunk + G + 2) * sizeof(uint32_t))};
  /* DC's and AC_exact's compressed pieces wait on the host until bin_index's length is known */
  unsigned char *dcz = (unsigned char *)host_buf(1, G * bound[1]), *acz = (unsigned char *)host_buf(2, G * bound[2]);
  drain_piece *pieces = (drain_piece *)malloc((3 * G + 3) * sizeof(drain_piece));
  if (!ix[0] || !ix[1] || !ix[2] || !pieces) { fprintf(stderr, "Out of memory: chunk index\n"); exit(1); }
  unsigned char *zc = dzc_sections(var_bytes(var_z));

  const double t0 = now_s();
  if (dctzhip_h2d_pipe_begin(c, g_dev.in, host_in, n * ts, gel * ts) != DCTZHIP_OK) die("H2D pipe");
  /* max|x|, min|x| of the whole array (util.c:18-25) */
  int T = host_threads();
  if (T > 64) T = 64;
  /* threads of the max|x| pass / of the follower: the call is bound by the HOST's memory traffic (the copy's staging, the
   * max|x| pass and the division together move six times the array: 250 GB/s on the measured host), more threads only take
   * bandwidth from the copy (tools/cpipe_sweep.py) */
  int TM = T < 16 ? T : 16, TF = T < 12 ? T : 12;
  { const char *e = getenv("DCTZ_PIPE_MM_THREADS"); if (e && atoi(e) > 0) TM = atoi(e) > 64 ? 64 : atoi(e); }
  { const char *e = getenv("DCTZ_PIPE_FOLLOW_THREADS"); if (e && atoi(e) > 0) TF = atoi(e) > 64 ? 64 : atoi(e); }
  mm_job mj[64];
  pthread_t mth[64];
  int mstarted = 0;
  for (int t = 0; t < TM; t++) {
    mj[t].x = host_in; mj[t].is_d = is_d; mj[t].lo = n / (size_t)TM * (size_t)t; mj[t].hi = t + 1 == TM ? n : n / (size_t)TM * (size_t)(t + 1);
    mj[t].mx = -1.0; mj[t].mn = INFINITY;
    if (t + 1 < TM && pthread_create(&mth[mstarted], NULL, mm_main, &mj[t]) == 0) mstarted++; else mm_main(&mj[t]);
  }
  for (int t = 0; t < mstarted; t++) pthread_join(mth[t], NULL);
  double mx = -1.0, mn = INFINITY;
  for (int t = 0; t < TM; t++) { if (mj[t].mx > mx) mx = mj[t].mx; if (mj[t].mn < mn) mn = mj[t].mn; }
  if (!(mx >= 0.0)) { mx = 0.0; mn = 0.0; }             /* (nothing but NaNs behind a finite first element: as the serial loop, max = |x[0]|) */
  { const double a0 = fabs(firsts[0]); if (a0 > mx) mx = a0; if (a0 < mn) mn = a0; }
  const double t_mm = now_s();

  drain_job dj;
  memset(&dj, 0, sizeof(dj));
  dj.c = c; dj.q = pieces; dj.cap = 3 * G + 3;
  dj.base[0] = zc; dj.base[1] = dcz; dj.base[2] = acz;
  pthread_t dth;
  if (pthread_create(&dth, NULL, drain_main, &dj)) { fprintf(stderr, "Error creating thread\n"); exit(0); }
  size_t npieces = 0, S = 0, ac_done = 0;                 /* pieces posted; exact coefficients so far; bytes of AC_exact deflated so far */
  double sum = 0.0, sf = 1.0, t_gpu = 0.0, t_tail = 0.0;
  follow_job fj = {host_in, n, is_d, 1.0, 0, 0, 0};
  track_job tj = {c, &fj, gel, ts};
  pthread_t fth[64], tth;
  int fstarted = 0, tracking = 0;
  for (size_t g = 0; g < G; g++) {
    const size_t e0 = g * gel, ne = n - e0 < gel ? n - e0 : gel, b0 = e0 / BLK_SZ, nb = CEIL(ne, BLK_SZ);
    const double tg0 = now_s();
    if (dctzhip_h2d_pipe_wait(c, (e0 + ne) * ts) != DCTZHIP_OK) die("H2D pipe");
    uint32_t cnt_g = 0;
    double pst[3];
    if (dctzhip_compress_part(c, (const char *)g_dev.in + e0 * ts, ne, dtype, error_bound, mx, mn, (unsigned char *)g_dev.bin + e0,
                              (float *)g_dev.dc + b0, (float *)g_dev.ac + S, &cnt_g, pst, &sf) != DCTZHIP_OK) die("dctzhip_compress_part");
    sum += pst[2] + (g ? firsts[g] : 0.0);
    S += cnt_g;
    const double tg1 = now_s();
    if (g == 0 && sf != 1.0 && scale_on_host(1)) {        /* the in-place x /= sf follows the copy from here on */
      fj.sf = sf;
      if (pthread_create(&tth, NULL, track_main, &tj) == 0) tracking = 1;
      for (int t = 0; tracking && t < TF; t++) if (pthread_create(&fth[fstarted], NULL, follow_worker, &fj) == 0) fstarted++;
    }
    /* the group's bin_index and DC, and the chunks of AC_exact that are complete by now (all of the rest behind the last group) */
    size_t ac_upto = S * sizeof(float);
    if (g + 1 < G) ac_upto -= ac_upto % chunk;
    const int nsec = ac_upto > ac_done ? 3 : 2;
    const void *gsrc[3] = {(const unsigned char *)g_dev.bin + e0, (const float *)g_dev.dc + b0, (const unsigned char *)g_dev.ac + ac_done};
    const size_t gn[3] = {ne, nb * sizeof(float), ac_upto - ac_done};
    void *gdst[3] = {(unsigned char *)g_dev.z[0] + g * bound[0], (unsigned char *)g_dev.z[1] + g * bound[1], (unsigned char *)g_dev.z[2] + g * bound[2]};
    uint32_t *gix[3] = {ix[0] + g * bpg, ix[1] + g * dpg, ix[2] + ac_done / chunk};
    const unsigned gflags[3] = {0u, DCTZHIP_DEFLATE_LITERALS, DCTZHIP_DEFLATE_LITERALS};   /* DC and AC_exact are bytes of floats */
    size_t glen[3] = {0, 0, 0};
    if (dctzhip_deflate_ex(c, nsec, gsrc, gn, gdst, bound, glen, gix, gflags) != DCTZHIP_OK) die("dctzhip_deflate");
    const size_t first_new = npieces;
    for (int i = 0; i < nsec; i++) {
      pieces[npieces].src = (const unsigned char *)gdst[i]; pieces[npieces].len = glen[i]; pieces[npieces].raw = gn[i]; pieces[npieces].sec = i;
      npieces++;
    }
    if (g + 1 == G && S == 0) {                            /* no exact coefficient at all: the empty stream, as the one call writes it */
      const size_t zero = 0;
      const void *asrc[1] = {g_dev.ac};
      void *adst[1] = {g_dev.z[2]};
      uint32_t *aix[1] = {ix[2]};
      size_t alen = 0;
      if (dctzhip_deflate_ex(c, 1, asrc, &zero, adst, &bound[2], &alen, aix, NULL) != DCTZHIP_OK) die("dctzhip_deflate");
      pieces[npieces].src = (const unsigned char *)g_dev.z[2]; pieces[npieces].len = alen; pieces[npieces].raw = 0; pieces[npieces].sec = 2;
      npieces++;
    }
    if (g + 1 == G) {
      /* The lengths of all three streams are known now -- what the drainer has brought back plus these last pieces --, so
       * DC's and AC_exact's last pieces go straight to their final places behind bin_index, and what is staged of them is
       * moved there by this thread while the drainer is busy with the last group. */
      while (__atomic_load_n(&dj.done, __ATOMIC_ACQUIRE) < first_new) { if (__atomic_load_n(&dj.failed, __ATOMIC_ACQUIRE)) die("D2H compressed pieces"); usleep(10); }
      size_t fin[3] = {dj.off[0], dj.off[1], dj.off[2]};
      int st[3] = {dj.started[0], dj.started[1], dj.started[2]};
      for (size_t k = first_new; k < npieces; k++) {
        if (pieces[k].len < 8) die("deflate: short stream");
        fin[pieces[k].sec] += pieces[k].len - (st[pieces[k].sec] ? 2 : 0) - 6;
        st[pieces[k].sec] = 1;
      }
      const size_t staged1 = dj.off[1], staged2 = dj.off[2];
      dj.base[1] = zc + fin[0] + 6;
      dj.base[2] = zc + fin[0] + 6 + fin[1] + 6;
      __atomic_store_n(&dj.posted, npieces, __ATOMIC_RELEASE);
      par_memcpy(dj.base[1], dcz, staged1, 4);
      par_memcpy(dj.base[2], acz, staged2, 8);
    } else
      __atomic_store_n(&dj.posted, npieces, __ATOMIC_RELEASE);
    ac_done = ac_upto;
    const double tg2 = now_s();
    t_gpu += tg1 - tg0; t_tail += tg2 - tg1;
    if (dbg) fprintf(stderr, "[cpipe] group %zu: start %.2f ms, wait + kernels %.2f, deflate %.2f (cnt %u), landed %zu\n", g, (tg0 - t0) * 1e3, (tg1 - tg0) * 1e3, (tg2 - tg1) * 1e3, cnt_g,
                     __atomic_load_n(&fj.landed, __ATOMIC_RELAXED) / gel);
  }
  ix_n[2] = (S * sizeof(float) + chunk - 1) / chunk;
  const double t_loop = now_s();
  __atomic_store_n(&dj.closed, 1, __ATOMIC_RELEASE);
  pthread_join(dth, NULL);
  if (dj.failed) die("D2H compressed pieces");
  if (dctzhip_h2d_pipe_end(c, 0) != DCTZHIP_OK) die("H2D pipe");
  const double t_drain = now_s();
  /* close the three streams (03 00 | adler32 of the whole section) and put DC's and AC_exact's behind bin_index's */
  size_t zlen[3];
  for (int i = 0; i < 3; i++) {
    unsigned char *t = dj.base[i] + dj.off[i];
    t[0] = 0x03; t[1] = 0x00; put_be32(t + 2, dj.adler[i]);
    zlen[i] = dj.off[i] + 6;
  }
  const size_t z0 = zlen[0], z1 = zlen[1], z2 = zlen[2];
  if (z0 > 0xffffffffu || z1 > 0xffffffffu || z2 > 0xffffffffu) { fprintf(stderr, "libdctz: a compressed section exceeds the header's 32-bit sizes (dctz.h:104-113): shard the array\n"); exit(1); }
  if (dj.base[1] != zc + z0 || dj.base[2] != zc + z0 + z1) die("pipelined compress: section lengths do not add up");
  const double t_asm = now_s();
  for (int t = 0; t < fstarted; t++) pthread_join(fth[t], NULL);
  if (tracking) pthread_join(tth, NULL);
  if (fj.failed) die("H2D pipe (follower)");
  if (sf != 1.0 && !fstarted) {                            /* (no follower thread could be started, or DCTZ_SCALE_HOST=0: the device's copy) */
    if (dctzhip_scale_inplace(c, g_dev.in, n, dtype, sf) != DCTZHIP_OK) die("scale");
    if (dctzhip_memcpy_d2h(c, host_in, g_dev.in, n * ts) != DCTZHIP_OK) die("D2H scaled input");
  }

  /* container: header | bin_indexz | DCz | AC_exactz | "DZIX"; the mean is util.c:28 / :41 on a tree-order sum (DCTZ_FAST_MEAN) */
  const dzc_desc d = {.type = var->datatype, .n = n, .npos = n, .error_bound = error_bound, .sf = sf, .cnt = (unsigned int)S,
                      .mean = is_d ? sum / (double)(int)n : (double)((float)sum / (float)(int)n), .zlen = {z0, z1, z2},
                      .chunk = chunk, .ix_n = ix_n, .ix = ix};
  *outSize = dzc_finish(var_bytes(var_z), &d);
  for (int i = 0; i < 3; i++) free(ix[i]);
  free(firsts); free(pieces);
  const double t_end = now_s();
  /* the stages overlap: h2d_s is the span up to the last group's kernels, gpu_s / zlib_s what the calling thread spent in the
   * groups' kernels / entropy stage, d2h_s what was left behind the last group (drain, assembly, the follower) */
  g_times.h2d_s = t_loop - t0; g_times.gpu_s = t_gpu; g_times.zlib_s = t_tail; g_times.d2h_s = t_end - t_loop;
  g_times.total_s = t_end - t_begin;
  if (dbg) fprintf(stderr, "[cpipe] max|x| at %.2f ms, last group queued %.2f, pieces drained %.2f, assembled %.2f, follower joined %.2f\n", (t_mm - t0) * 1e3, (t_loop - t0) * 1e3,
                   (t_drain - t0) * 1e3, (t_asm - t0) * 1e3, (t_end - t0) * 1e3);
  if (!quiet()) printf("outSize = %zu\n", *outSize); /* :841-843 */
  return 1;
}

/* -------------------------------------------------------------- compress --- */
int dctz_compress(t_var *var, int N, size_t *outSize, t_var *var_z, double error_bound) {
  const double t_begin = now_s();
  const int is_d = (var->datatype == DOUBLE);
  const size_t ts = is_d ? sizeof(double) : sizeof(float);
  const int dtype = is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  void *host_in = var_bytes(var);

  if (error_bound < 1E-6) { /* dctz-comp-lib.c:135-138 */
    printf("ERROR BOUND is not acceptable");
    exit(1);
  }
  if (N <= 0) { fprintf(stderr, "libdctz: N must be positive\n"); exit(1); }
  const size_t n = (size_t)N;
  size_t dims[3] = {0, 0, 0};
  const int nd = take_block_dims(n, dims);      /* 0: the reference's flat blocks */
  size_t nblk = CEIL(n, BLK_SZ);
  if (nd) {
    nblk = dctzhip_nd_blocks(nd, dims);
    if (!nblk) { fprintf(stderr, "libdctz: array too large for multi-dimensional blocks\n"); exit(1); }
  }
  const size_t npos = nd ? nblk * BLK_SZ : n;   /* positions the streams cover (edge tiles are padded) */

  dctzhip_ctx *c = ctx();
  if (!nd && zlib_gpu() && fast_mean() && pipeline_on() && !getenv("DCTZ_DUMP_STREAMS") &&
      compress_pipelined(c, var, host_in, n, is_d, error_bound, var_z, outSize, t_begin)) return 1;
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.bin, &g_dev.bin_cap, npos);
  grow(&g_dev.dc, &g_dev.dc_cap, nblk * sizeof(float));
  grow(&g_dev.ac, &g_dev.ac_cap, npos * sizeof(float));

  /* util.c:18-19 starts max and min from |x[0]|: a NaN there stays (no comparison against it is true), sf = NaN, and the
   * in-place x /= sf (dctz-comp-lib.c:193-216) has made the whole array NaN before the first block is transformed.  The
   * drop-in keeps that rule (the device ABI passes a NaN over wherever it stands), the way the
   * reference gets there: the mean of the array as it came (util.c:22 never adds x[0]), then the division -- the device
   * compresses the array of NaNs, and the header says sf = NaN. */
  const int nan_first = is_d ? isnan(((const double *)host_in)[0]) : isnan(((const float *)host_in)[0]);
  double nan_first_mean = 0.0;
  if (nan_first) {
    host_mean_job m0 = {host_in, n, is_d, 0.0, 0};
    (void)host_mean_main(&m0);
    nan_first_mean = m0.mean;
    if (is_d) { double *x = (double *)host_in; for (size_t i = 0; i < n; i++) x[i] /= (double)NAN; }
    else { float *x = (float *)host_in; for (size_t i = 0; i < n; i++) x[i] /= (float)NAN; }
  }

  double t0 = now_s();
  if (dctzhip_memcpy_h2d(c, g_dev.in, host_in, n * ts) != DCTZHIP_OK) die("H2D");
  double t1 = now_s();

  /* a2..a9 on the GPU; the scaled array is produced in place on the device and
   * copied back over the caller's buffer (the reference's in-place "/= sf") */
  dctzhip_cinfo info;
  const int gpu_tail = zlib_gpu();
  const int fast_tail = gpu_tail || zlib_threads() > 3;
  pthread_t mean_thread;
  host_mean_job mj = {host_in, n, is_d, 0.0, 0};
  int mean_on_host = 0;
  const int tree_mean = fast_mean();
  if (!tree_mean && fast_tail && pthread_create(&mean_thread, NULL, host_mean_main, &mj) == 0) mean_on_host = 1;
  if (!tree_mean && !mean_on_host && dctzhip_serial_mean_begin(c, g_dev.in, n, dtype) != DCTZHIP_OK) die("serial mean");
  int rc = nd ? dctzhip_compress_nd(c, g_dev.in, nd, dims, dtype, error_bound, DCTZ_MODE, g_dev.bin, (float *)g_dev.dc,
                                    (float *)g_dev.ac, NULL, &info)
              : dctzhip_compress(c, g_dev.in, n, dtype, error_bound, DCTZ_MODE, g_dev.bin, (float *)g_dev.dc,
                                 (float *)g_dev.ac, NULL, NULL, &info);
  if (rc != DCTZHIP_OK) die("dctzhip_compress");
  if (nan_first) info.sf = (double)NAN;             /* (the array is all NaN by now: the device said sf = 1 and scaled nothing) */
  if (dctzhip_sync(c) != DCTZHIP_OK) die("sync");   /* (the call returns while its last kernels drain: keep the stage timers honest) */
  double t2 = now_s();

  /* raw streams on the host: what the host zlib tails read, and what the dump taps write */
  const int want_raw = !gpu_tail || getenv("DCTZ_DUMP_STREAMS") != NULL;
  t_bin_id *bin_index = NULL;
  float *DC = NULL, *AC_exact = NULL;
  if (want_raw) {
    bin_index = (t_bin_id *)host_buf(0, npos);
    DC = (float *)host_buf(1, nblk * sizeof(float));
    AC_exact = (float *)host_buf(2, (size_t)info.cnt * sizeof(float));
    if (dctzhip_memcpy_d2h(c, bin_index, g_dev.bin, npos) != DCTZHIP_OK) die("D2H bin_index");
    if (dctzhip_memcpy_d2h(c, DC, g_dev.dc, nblk * sizeof(float)) != DCTZHIP_OK) die("D2H DC");
    if (info.cnt && dctzhip_memcpy_d2h(c, AC_exact, g_dev.ac, (size_t)info.cnt * sizeof(float)) != DCTZHIP_OK)
      die("D2H AC_exact");
  }
  double t3 = now_s();

  if (getenv("DCTZ_DUMP_STREAMS")) { /* dctz-comp-lib.c:583-595, :443-448 */
    dump_file("bin_index.bin", bin_index, npos);
    dump_file("AC_exact.bin", AC_exact, (size_t)info.cnt * sizeof(float));
#ifdef USE_QTABLE
    if (is_d) dump_file("qtable.bin", info.qtable_raw, BLK_SZ * sizeof(double));
    else { float q[BLK_SZ]; for (int j = 0; j < BLK_SZ; j++) q[j] = (float)info.qtable_raw[j]; dump_file("qtable.bin", q, sizeof(q)); }
#endif
  }

  /* zlib tail: three streams on three threads (dctz-comp-lib.c:620-732) */
  const int zthreads = zlib_threads();
  const size_t sec_bytes[3] = {npos * sizeof(t_bin_id), nblk * sizeof(float), (size_t)info.cnt * sizeof(float)};
  const void *sec_src[3] = {bin_index, DC, AC_exact};
  pthread_attr_t attr;
  pthread_attr_init(&attr);
  pthread_attr_setdetachstate(&attr, PTHREAD_CREATE_JOINABLE);
  zjob jb[3];
  memset(jb, 0, sizeof(jb));
  pthread_t pd_thread;
  pd_args pda;
  size_t pd_len[3] = {0, 0, 0};
  size_t gz_len[3] = {0, 0, 0};
  double t_gz = 0.0;                        /* end of the device entropy stage (the write-back of x/sf follows it) */
  uint32_t *ix[3] = {NULL, NULL, NULL};     /* compressed bytes per chunk, for the "DZIX" trailer */
  size_t ix_n[3] = {0, 0, 0};
  const int host_scale = scale_on_host(gpu_tail) && info.sf != 1.0 && !nan_first;
  pthread_t scale_thread;
  scale_mgr sm = {host_in, n, is_d, host_threads(), info.sf, mean_on_host ? &mean_thread : NULL, mean_on_host ? &mj : NULL, 0};
  int scale_started = 0;
  if (host_scale && pthread_create(&scale_thread, NULL, scale_mgr_main, &sm) == 0) scale_started = 1;
  if (gpu_tail) {                           /* deflate on the device, compressed bytes only over PCIe */
    const void *gsrc[3] = {g_dev.bin, g_dev.dc, g_dev.ac};
    size_t gcap[3];
    for (int i = 0; i < 3; i++) {
      gcap[i] = dctzhip_deflate_bound(sec_bytes[i]);
      grow(&g_dev.z[i], &g_dev.z_cap[i], gcap[i]);
      ix_n[i] = (sec_bytes[i] + dctzhip_deflate_chunk_bytes() - 1) / dctzhip_deflate_chunk_bytes();
      ix[i] = (uint32_t *)malloc((ix_n[i] ? ix_n[i] : 1) * sizeof(uint32_t));
      if (!ix[i]) { fprintf(stderr, "Out of memory: chunk index\n"); exit(1); }
    }
    const unsigned gflags[3] = {0u, DCTZHIP_DEFLATE_LITERALS, DCTZHIP_DEFLATE_LITERALS};   /* DC and AC_exact are bytes of floats */
    if (dctzhip_deflate_ex(c, 3, gsrc, sec_bytes, (void *const *)g_dev.z, gcap, gz_len, (uint32_t *const *)ix, gflags) != DCTZHIP_OK) die("dctzhip_deflate");
    /* the sections go straight from the device into the caller's container, behind the header (:775-820) */
    unsigned char *zc = dzc_sections(var_bytes(var_z));
    for (int i = 0; i < 3; i++) {
      if (dctzhip_memcpy_d2h(c, zc, g_dev.z[i], gz_len[i]) != DCTZHIP_OK) die("D2H compressed section");
      zc += gz_len[i];
    }
    t_gz = now_s();
  } else if (zthreads > 3) {                /* chunked deflate, one pool for all three sections */
    for (int i = 0; i < 3; i++) {
      jb[i].bound = (uLong)dctz_pdeflate_bound(sec_bytes[i], zlib_chunk());
      jb[i].dst = (Bytef *)malloc(jb[i].bound);
      if (!jb[i].dst) { fprintf(stderr, "Out of memory: zlib buffer\n"); exit(1); }
      pda.sec[i].src = sec_src[i]; pda.sec[i].n = sec_bytes[i];
      pda.sec[i].dst = jb[i].dst; pda.sec[i].cap = jb[i].bound; pda.sec[i].out_len = &pd_len[i];
    }
    pda.threads = zthreads; pda.chunk = zlib_chunk(); pda.rc = 0;
    { const char *e = getenv("DCTZ_ZLIB_LEVEL"); dctz_pdeflate_set_level(e ? atoi(e) : -1); }
    if (pthread_create(&pd_thread, &attr, pd_main, &pda)) { fprintf(stderr, "Error creating thread\n"); exit(0); }
  } else {
    for (int i = 0; i < 3; i++) zjob_start(&jb[i], sec_src[i], sec_bytes[i], &attr);
  }

  /* while zlib runs: write x/sf back over the caller's buffer (:193-216) and
   * fetch the serial-order mean for the header */
  double mean_serial = 0.0;
  if (scale_started) pthread_join(scale_thread, NULL);                            /* (it has joined the mean thread itself) */
  else if (mean_on_host) pthread_join(mean_thread, NULL);                         /* before host_in is overwritten */
  if (tree_mean) mean_serial = info.mean;
  else if (mean_on_host) mean_serial = mj.mean;
  else if (dctzhip_serial_mean_end(c, &mean_serial) != DCTZHIP_OK) die("serial mean");
  if (nan_first) mean_serial = nan_first_mean;
  if (info.sf != 1.0 && !scale_started && !nan_first) {   /* only now may the device copy of the input change */
    if (dctzhip_scale_inplace(c, g_dev.in, n, dtype, info.sf) != DCTZHIP_OK) die("scale");
    if (dctzhip_memcpy_d2h(c, host_in, g_dev.in, n * ts) != DCTZHIP_OK) die("D2H scaled input");
  }

  uLong zsz[3];
  if (gpu_tail) {
    for (int i = 0; i < 3; i++) zsz[i] = (uLong)gz_len[i];
  } else if (zthreads > 3) {
    pthread_join(pd_thread, NULL);
    if (pda.rc) { fprintf(stderr, "libdctz: parallel deflate failed (%d)\n", pda.rc); exit(1); }
    for (int i = 0; i < 3; i++) zsz[i] = (uLong)pd_len[i];
  } else {
    for (int i = 0; i < 3; i++) zsz[i] = zjob_join(&jb[i]);
  }
  for (int i = 0; i < 3; i++)
    if (zsz[i] > 0xffffffffu) { fprintf(stderr, "libdctz: compressed section %d is %lu bytes; the header holds 32-bit sizes (dctz.h:104-113): shard the array\n", i, zsz[i]); exit(1); }
  pthread_attr_destroy(&attr);
  double t4 = now_s();

  /* container: header | bin_indexz | DCz | AC_exactz | [qtable] | ["DZND"] | ["DZIX"]  (:775-820) */
  if (!gpu_tail) {                             /* (the device's sections are already in place) */
    unsigned char *cur = dzc_sections(var_bytes(var_z));
    for (int i = 0; i < 3; i++) { memcpy(cur, jb[i].dst, zsz[i]); cur += zsz[i]; }
  }
  const dzc_desc d = {.type = var->datatype, .nd = nd, .dims = dims, .n = n, .npos = npos, .error_bound = error_bound, .sf = info.sf,
                      .mean = mean_serial, .cnt = info.cnt, .zlen = {zsz[0], zsz[1], zsz[2]},
                      .qtable = DCTZ_QT ? info.qtable : NULL,
                      .chunk = dctzhip_deflate_chunk_bytes(), .ix_n = ix_n, .ix = gpu_tail ? ix : NULL};
  *outSize = dzc_finish(var_bytes(var_z), &d);
  for (int i = 0; i < 3; i++) free(ix[i]);
  for (int i = 0; i < 3; i++) free(jb[i].dst);

  g_times.h2d_s = t1 - t0; g_times.gpu_s = t2 - t1; g_times.d2h_s = t3 - t2; g_times.zlib_s = t4 - t3;
  if (gpu_tail) { g_times.zlib_s = t_gz - t3; g_times.d2h_s += t4 - t_gz; }   /* nothing overlaps the write-back of x/sf here: count it as the copy it is */
  g_times.total_s = now_s() - t_begin;
  if (!quiet()) printf("outSize = %zu\n", *outSize); /* :841-843 */
  return 1;
}

/* ---- lists of arrays in host memory (round 4; ADDITIONS to the reference's API, include/dctz.h) ---------------------------
 * The reference's own workloads are lists of small arrays, one dctz_compress() call -- one process -- per array
 * (tests/test-dctz.sh:13-56 over tests/list-msst19.txt:1-6).  Through this drop-in one such call is an H2D copy, one kernel,
 * a D2H copy and three zlib threads around a few microseconds of GPU work; k of them in a loop are k times that.
 * dctz_compress_batch() takes the k arrays at once: ONE staged H2D copy, ONE batch launch (dctzhip_compress_batch: every
 * array with its own statistics, scaling factor, bin ranges and tot_AC_exact_count, as in its own call), ONE copy back, and
 * the 3 k single-shot deflates of the reference's tail (dctz-comp-lib.c:620-732, same parameters) dealt to a pool of host
 * threads together with the k in-place scalings (:193-216) and serial-order means (util.c:18-28).  Every container is byte
 * for byte the one dctz_compress() writes for that array (reference tail), every caller's array ends up divided by its sf. */
typedef struct {
  int kind;                     /* 0: deflate one section, 1: scale + mean of one array, 2: inflate one section */
  int arr, sec;
  const void *src; size_t n;    /* deflate / inflate input */
  Bytef *dst; uLong cap, out;   /* ... output */
  void *x; size_t nx; int is_d; double sf, mean;
  int rc;
} bjob;
typedef struct { bjob *jobs; size_t njobs, next; } bpool;
static void bjob_run(bjob *j) {
  if (j->kind == 0) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    /* dctz-comp-lib.c:642-643: default level, 32K window, memLevel 8, default strategy; one deflate(Z_FINISH) (:75-88) */
    if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 15, DEF_MEM_LEVEL, Z_DEFAULT_STRATEGY) != Z_OK) { j->rc = 1; return; }
    zs.data_type = Z_UNKNOWN;
    zs.next_in = (Bytef *)j->src; zs.avail_in = (uInt)j->n;
    zs.next_out = j->dst; zs.avail_out = (uInt)j->cap;
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) j->rc = 1;
    j->out = zs.total_out;
    deflateEnd(&zs);
  } else if (j->kind == 2) {
    j->out = inflate_into((const Bytef *)j->src, (uLong)j->n, j->dst, (size_t)j->cap);
  } else {
    /* the header's mean in the reference's order (util.c:18-28 / :31-41), then the in-place x /= sf (:193-216) */
    if (j->is_d) {
      double *x = (double *)j->x, sum = 0.0;
      for (size_t i = 1; i < j->nx; i++) sum += x[i];
      j->mean = sum / (double)(int)j->nx;
      if (j->sf != 1.0) for (size_t i = 0; i < j->nx; i++) x[i] /= j->sf;
    } else {
      float *x = (float *)j->x, sum = 0.0f;
      const float sf = (float)j->sf;
      for (size_t i = 1; i < j->nx; i++) sum += x[i];
      j->mean = (double)(sum / (float)(int)j->nx);
      if (sf != 1.0f) for (size_t i = 0; i < j->nx; i++) x[i] /= sf;
    }
  }
}
static void *bpool_worker(void *arg) {
  bpool *p = (bpool *)arg;
  for (;;) {
    const size_t i = __atomic_fetch_add(&p->next, 1, __ATOMIC_RELAXED);
    if (i >= p->njobs) break;
    bjob_run(&p->jobs[i]);
  }
  return NULL;
}
static void bpool_run(bjob *jobs, size_t njobs) {
  bpool p = {jobs, njobs, 0};
  int T = host_threads();
  if ((size_t)T > njobs) T = (int)njobs;
  pthread_t th[64];
  if (T > 64) T = 64;
  int started = 0;
  for (int t = 1; t < T; t++) { if (pthread_create(&th[started], NULL, bpool_worker, &p) == 0) started++; }
  bpool_worker(&p);
  for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
}
/* --------------------------------------------------- compress to a target PSNR (ADDITION, dctz.h) --- */
/* The array goes to the device, dctzhip_compress_psnr chooses the bound (include/dctz_hip.h: probe, compress, measure,
 * step down), and the container is then simply dctz_compress(var, N, outSize, var_z, bound) -- byte for byte that call's
 * output, the in-place x /= sf of the caller's buffer included.  (The second H2D copy inside dctz_compress is the price of
 * that identity.)  EC only: the QT build refuses without touching anything. */
int dctz_compress_psnr(t_var *var, int N, size_t *outSize, t_var *var_z, double target_psnr, double *error_bound_used) {
#ifdef USE_QTABLE
  (void)var; (void)N; (void)outSize; (void)var_z; (void)target_psnr; (void)error_bound_used;
  return DCTZHIP_E_ARG;                          /* QT bin widths come from a whole-array table: no probe for them */
#else
  if (!var || !var_z || !outSize || !error_bound_used || N <= 0) return DCTZHIP_E_ARG;
  if (g_nd || (getenv("DCTZ_BLOCK_DIMS") && *getenv("DCTZ_BLOCK_DIMS"))) return DCTZHIP_E_ARG;   /* flat blocks only */
  const int is_d = (var->datatype == DOUBLE);
  if (!is_d && var->datatype != FLOAT) return DCTZHIP_E_ARG;
  const void *host_in = var_bytes(var);
  if (!host_in) return DCTZHIP_E_ARG;
  const size_t n = (size_t)N, ts = is_d ? sizeof(double) : sizeof(float);
  dctzhip_ctx *c = ctx();
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.bin, &g_dev.bin_cap, n);
  grow(&g_dev.dc, &g_dev.dc_cap, CEIL(n, BLK_SZ) * sizeof(float));
  grow(&g_dev.ac, &g_dev.ac_cap, n * sizeof(float));
  if (dctzhip_memcpy_h2d(c, g_dev.in, host_in, n * ts) != DCTZHIP_OK) die("H2D");
  dctzhip_cinfo info;
  double eb = 0.0, psnr = 0.0;
  const int rc = dctzhip_compress_psnr(c, g_dev.in, n, is_d ? DCTZHIP_F64 : DCTZHIP_F32, target_psnr, g_dev.bin, (float *)g_dev.dc,
                                       (float *)g_dev.ac, &info, &eb, &psnr);
  if (rc != DCTZHIP_OK) return rc;
  *error_bound_used = eb;
  return dctz_compress(var, N, outSize, var_z, eb);
#endif
}

/* The same for an array compressed in tiles: dctzhip_compress_psnr_nd chooses the bound, and the container is byte for byte
 * dctz_set_block_dims(ndims, dims) + dctz_compress(var, prod dims, outSize, var_z, bound).  A request of the caller's that is
 * still pending is not consumed: the call is refused.  Every refusal that does not need the data comes before a device is
 * asked for. */
int dctz_compress_psnr_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, double target_psnr,
                          double *error_bound_used) {
#ifdef USE_QTABLE
  (void)var; (void)ndims; (void)dims; (void)outSize; (void)var_z; (void)target_psnr; (void)error_bound_used;
  return DCTZHIP_E_ARG;                          /* QT bin widths come from a whole-array table: no probe for them */
#else
  if (!var || !var_z || !outSize || !error_bound_used) return DCTZHIP_E_ARG;
  if ((ndims != 2 && ndims != 3) || !dims || g_nd) return DCTZHIP_E_ARG;
  const int is_d = (var->datatype == DOUBLE);
  if (!is_d && var->datatype != FLOAT) return DCTZHIP_E_ARG;
  const void *host_in = var_bytes(var);
  if (!host_in || isnan(target_psnr) || isinf(target_psnr)) return DCTZHIP_E_ARG;
  size_t n = 1;
  for (int i = 0; i < ndims; i++) {
    if (dims[i] == 0 || dims[i] > 0x7FFFFFFFu || n > (size_t)0x7FFFFFFF / dims[i]) return DCTZHIP_E_ARG;
    n *= dims[i];
  }
  const size_t nblk = dctzhip_nd_blocks(ndims, dims);
  if (nblk == 0) return DCTZHIP_E_ARG;             /* (more tiles than the streams can number) */
  const size_t ts = is_d ? sizeof(double) : sizeof(float);
  dctzhip_ctx *c = ctx();
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.bin, &g_dev.bin_cap, nblk * BLK_SZ);
  grow(&g_dev.dc, &g_dev.dc_cap, nblk * sizeof(float));
  grow(&g_dev.ac, &g_dev.ac_cap, nblk * BLK_SZ * sizeof(float));
  if (dctzhip_memcpy_h2d(c, g_dev.in, host_in, n * ts) != DCTZHIP_OK) die("H2D");
  dctzhip_cinfo info;
  double eb = 0.0, psnr = 0.0;
  const int rc = dctzhip_compress_psnr_nd(c, g_dev.in, ndims, dims, is_d ? DCTZHIP_F64 : DCTZHIP_F32, target_psnr, g_dev.bin,
                                          (float *)g_dev.dc, (float *)g_dev.ac, &info, &eb, &psnr);
  if (rc != DCTZHIP_OK) return rc;
  if (dctz_set_block_dims(ndims, dims) != 0) return DCTZHIP_E_ARG;
  *error_bound_used = eb;
  return dctz_compress(var, (int)n, outSize, var_z, eb);
#endif
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
static struct { void *pin; size_t pin_cap; void *dev; size_t dev_cap; } g_batch;
static void batch_buffers(dctzhip_ctx *c, size_t host_bytes, size_t dev_bytes) {
  if (host_bytes > g_batch.pin_cap) {
    if (g_batch.pin) dctzhip_host_unregister(c, g_batch.pin), free(g_batch.pin);
    g_batch.pin = NULL; g_batch.pin_cap = 0;
    if (posix_memalign(&g_batch.pin, 4096, host_bytes)) { fprintf(stderr, "Out of memory: batch staging\n"); exit(1); }
    memset(g_batch.pin, 0, host_bytes);
    (void)dctzhip_host_register(c, g_batch.pin, host_bytes);      /* (pinned: one fast copy each way; unpinned it still works) */
    g_batch.pin_cap = host_bytes;
  }
  grow(&g_batch.dev, &g_batch.dev_cap, dev_bytes);
}

/* Caller arrays that share bytes (one t_var twice, two t_vars over one buffer): the second call of the loop reads what the
 * first one's in-place scaling left there, which the pool -- sums and divisions of all arrays at once -- cannot reproduce.
 * Such a list is run as that loop; the sort makes the check O(k log k). */
typedef struct { uintptr_t lo, hi; } brange;
static int brange_cmp(const void *a, const void *b) {
  const uintptr_t x = ((const brange *)a)->lo, y = ((const brange *)b)->lo;
  return x < y ? -1 : x > y;
}
static int batch_inputs_overlap(int k, t_var *const *vars, const int *N) {
  brange *r = (brange *)malloc((size_t)k * sizeof(*r));
  if (!r) { fprintf(stderr, "Out of memory: batch\n"); exit(1); }
  for (int i = 0; i < k; i++) {
    const int is_d = vars[i]->datatype == DOUBLE;
    r[i].lo = (uintptr_t)var_bytes(vars[i]);
    r[i].hi = r[i].lo + (size_t)(N[i] > 0 ? N[i] : 0) * (is_d ? 8 : 4);
  }
  qsort(r, (size_t)k, sizeof(*r), brange_cmp);
  int hit = 0;
  uintptr_t end = 0;
  for (int i = 0; i < k && !hit; i++) {
    if (r[i].hi == r[i].lo) continue;
    hit = i > 0 && end > r[i].lo;
    if (r[i].hi > end) end = r[i].hi;
  }
  free(r);
  return hit;
}

int dctz_compress_batch(int k, t_var *const *vars, const int *N, size_t *outSizes, t_var *const *vars_z, const double *error_bounds) {
  if (k <= 0) return 1;
  if (batch_inputs_overlap(k, vars, N)) {
    for (int i = 0; i < k; i++) if (dctz_compress(vars[i], N[i], &outSizes[i], vars_z[i], error_bounds[i]) != 1) return 0;
    return 1;
  }
  /* an array whose first element is a NaN: dctz_compress keeps util.c's rule for it (max = sf = NaN);
   * a list that holds one goes call by call */
  for (int i = 0; i < k; i++)
    if (N[i] > 0 && (vars[i]->datatype == DOUBLE ? isnan(((const double *)var_bytes(vars[i]))[0]) : isnan(((const float *)var_bytes(vars[i]))[0]))) {
      for (int q = 0; q < k; q++) if (dctz_compress(vars[q], N[q], &outSizes[q], vars_z[q], error_bounds[q]) != 1) return 0;
      return 1;
    }
  dctzhip_ctx *c = ctx();
  /* layout of the staging area (host, pinned) and of its device twin: inputs | bin_index | DC | AC_exact, array after array */
  size_t *off_in = (size_t *)malloc(4 * (size_t)k * sizeof(size_t));
  dctzhip_batch_citem *items = (dctzhip_batch_citem *)calloc((size_t)k, sizeof(*items));
  dctzhip_cinfo *infos = (dctzhip_cinfo *)calloc((size_t)k, sizeof(*infos));
  if (!off_in || !items || !infos) { fprintf(stderr, "Out of memory: batch\n"); exit(1); }
  size_t *off_bin = off_in + k, *off_dc = off_in + 2 * k, *off_ac = off_in + 3 * k;
  size_t in_bytes = 0, total = 0;
  for (int i = 0; i < k; i++) {
    if (error_bounds[i] < 1E-6) { printf("ERROR BOUND is not acceptable"); exit(1); }     /* dctz-comp-lib.c:135-138 */
    if (N[i] <= 0) { fprintf(stderr, "libdctz: N must be positive\n"); exit(1); }
    const size_t ts = vars[i]->datatype == DOUBLE ? 8 : 4;
    off_in[i] = in_bytes; in_bytes += up256((size_t)N[i] * ts);
  }
  total = in_bytes;
  for (int i = 0; i < k; i++) { off_bin[i] = total; total += up256((size_t)N[i]); }
  for (int i = 0; i < k; i++) { off_dc[i] = total; total += up256(CEIL((size_t)N[i], BLK_SZ) * sizeof(float)); }
  for (int i = 0; i < k; i++) { off_ac[i] = total; total += up256((size_t)N[i] * sizeof(float)); }
  batch_buffers(c, total, total);
  unsigned char *hp = (unsigned char *)g_batch.pin, *dp = (unsigned char *)g_batch.dev;
  for (int i = 0; i < k; i++) {
    const int is_d = vars[i]->datatype == DOUBLE;
    const size_t ts = is_d ? 8 : 4;
    memcpy(hp + off_in[i], var_bytes(vars[i]), (size_t)N[i] * ts);
    items[i].d_in = dp + off_in[i]; items[i].n = (size_t)N[i]; items[i].dtype = is_d ? DCTZHIP_F64 : DCTZHIP_F32;
    items[i].error_bound = error_bounds[i];
    items[i].d_bin_index = dp + off_bin[i]; items[i].d_dc = (float *)(dp + off_dc[i]); items[i].d_ac_exact = (float *)(dp + off_ac[i]);
    items[i].d_scaled = NULL;
  }
  if (dctzhip_memcpy_h2d(c, dp, hp, in_bytes) != DCTZHIP_OK) die("H2D (batch)");
  if (dctzhip_compress_batch(c, k, items, DCTZ_MODE, infos) != DCTZHIP_OK) die("dctzhip_compress_batch");
  if (dctzhip_memcpy_d2h(c, hp + in_bytes, dp + in_bytes, total - in_bytes) != DCTZHIP_OK) die("D2H (batch)");   /* (waits for the kernels first) */
  /* the tails: 3 k deflates + k (mean, scaling) jobs on the pool, the longest first */
  bjob *jobs = (bjob *)calloc(4 * (size_t)k, sizeof(bjob));
  if (!jobs) { fprintf(stderr, "Out of memory: batch\n"); exit(1); }
  size_t nj = 0;
  for (int pass = 0; pass < 4; pass++)                /* AC_exact sections first (bytes of floats: the slow ones), then bin_index, DC, scalings */
    for (int i = 0; i < k; i++) {
      const size_t n = (size_t)N[i], nblk = CEIL(n, BLK_SZ);
      bjob *j = &jobs[nj];
      j->arr = i;
      if (pass == 3) {
        const int is_d = vars[i]->datatype == DOUBLE;
        j->kind = 1; j->x = var_bytes(vars[i]); j->nx = n; j->is_d = is_d; j->sf = infos[i].sf;
      } else {
        const int sec = pass == 0 ? 2 : pass - 1;
        const size_t bytes = sec == 0 ? n : (sec == 1 ? nblk * sizeof(float) : (size_t)infos[i].cnt * sizeof(float));
        j->kind = 0; j->sec = sec; j->n = bytes;
        j->src = hp + (sec == 0 ? off_bin[i] : (sec == 1 ? off_dc[i] : off_ac[i]));
        j->cap = compressBound((uLong)bytes);
        j->dst = (Bytef *)malloc(j->cap ? j->cap : 1);
        if (!j->dst) { fprintf(stderr, "Out of memory: zlib buffer\n"); exit(1); }
      }
      nj++;
    }
  if (getenv("DCTZ_DUMP_STREAMS")) fprintf(stderr, "libdctz: DCTZ_DUMP_STREAMS is a tap of single calls; dctz_compress_batch writes no dump files\n");
  bpool_run(jobs, nj);
  /* containers: header | bin_indexz | DCz | AC_exactz | [qtable]  (:775-820) */
  for (int i = 0; i < k; i++) {
    const bjob *jz[3] = {NULL, NULL, NULL}, *js = NULL;
    for (size_t q = 0; q < nj; q++) if (jobs[q].arr == i) { if (jobs[q].kind == 1) js = &jobs[q]; else jz[jobs[q].sec] = &jobs[q]; }
    for (int s3 = 0; s3 < 3; s3++) if (jz[s3]->rc) { fprintf(stderr, "libdctz: deflate failed\n"); exit(1); }
    unsigned char *cur = dzc_sections(var_bytes(vars_z[i]));
    for (int s3 = 0; s3 < 3; s3++) { memcpy(cur, jz[s3]->dst, jz[s3]->out); cur += jz[s3]->out; }
    const dzc_desc d = {.type = vars[i]->datatype, .n = (size_t)N[i], .npos = (size_t)N[i], .error_bound = error_bounds[i], .sf = infos[i].sf,
                        .mean = js->mean, .cnt = infos[i].cnt, .zlen = {jz[0]->out, jz[1]->out, jz[2]->out},
                        .qtable = DCTZ_QT ? infos[i].qtable : NULL};
    const size_t out = dzc_finish(var_bytes(vars_z[i]), &d);
    outSizes[i] = out;
    if (!quiet()) printf("outSize = %zu\n", out); /* :841-843 */
  }
  for (size_t q = 0; q < nj; q++) free(jobs[q].dst);
  free(jobs); free(off_in); free(items); free(infos);
  return 1;
}

int dctz_decompress_batch(int k, t_var *const *vars_z, t_var *const *vars_r) {
  if (k <= 0) return 1;
  dctzhip_ctx *c = ctx();
  dzc_view *vs = (dzc_view *)malloc((size_t)k * sizeof(dzc_view));
  size_t *off_bin = (size_t *)malloc(4 * (size_t)k * sizeof(size_t));
  dctzhip_batch_ditem *items = (dctzhip_batch_ditem *)calloc((size_t)k, sizeof(*items));
  bjob *jobs = (bjob *)calloc(3 * (size_t)k, sizeof(bjob));
  double *qtabs = (double *)malloc((size_t)k * BLK_SZ * sizeof(double));
  if (!vs || !off_bin || !items || !jobs || !qtabs) { fprintf(stderr, "Out of memory: batch\n"); exit(1); }
  size_t *off_dc = off_bin + k, *off_ac = off_bin + 2 * k, *off_out = off_bin + 3 * k;
  size_t total = 0, in_bytes;
  for (int i = 0; i < k; i++) {
    dzc_header(&vs[i], var_bytes(vars_z[i]), DCTZ_QT, (int)vars_z[i]->datatype);
    if (vs[i].n == 0) { fprintf(stderr, "libdctz: empty stream\n"); exit(1); }
    if (vs[i].nd) { fprintf(stderr, "libdctz: dctz_decompress_batch takes flat containers\n"); exit(1); }
  }
  for (int i = 0; i < k; i++) { off_bin[i] = total; total += up256(vs[i].raw[0]); }
  for (int i = 0; i < k; i++) { off_dc[i] = total; total += up256(vs[i].raw[1]); }
  for (int i = 0; i < k; i++) { off_ac[i] = total; total += up256(vs[i].raw[2] + 4 * sizeof(float)); }
  in_bytes = total;
  for (int i = 0; i < k; i++) { off_out[i] = total; total += up256(vs[i].n * vs[i].ts); }
  batch_buffers(c, total, total);
  unsigned char *hp = (unsigned char *)g_batch.pin, *dp = (unsigned char *)g_batch.dev;
  size_t nj = 0;
  for (int i = 0; i < k; i++) {
    const dzc_view *v = &vs[i];
    const size_t offs[3] = {off_bin[i], off_dc[i], off_ac[i]};
    for (int s3 = 0; s3 < 3; s3++) {                                   /* three inflates per array (dctz-decomp-lib.c:244-322) */
      bjob *j = &jobs[nj++];
      j->kind = 2; j->arr = i; j->sec = s3; j->src = v->sec[s3]; j->n = v->zlen[s3]; j->dst = hp + offs[s3]; j->cap = (uLong)v->raw[s3];
    }
    items[i].d_bin_index = dp + off_bin[i]; items[i].d_dc = (const float *)(dp + off_dc[i]); items[i].d_ac_exact = (const float *)(dp + off_ac[i]);
    items[i].ac_count = v->cnt; items[i].qtable_host = dzc_qtable(v, qtabs + (size_t)i * BLK_SZ);
    items[i].n = v->n; items[i].dtype = v->is_d ? DCTZHIP_F64 : DCTZHIP_F32; items[i].error_bound = v->h.error_bound;
    items[i].sf = v->sf;
    items[i].d_out = dp + off_out[i];
  }
  bpool_run(jobs, nj);
  if (!quiet()) for (int i = 0; i < k; i++) printf("uncompressed bin_index size is: %lu\n", (unsigned long)jobs[3 * (size_t)i].out); /* :260-262 */
  if (dctzhip_memcpy_h2d(c, dp, hp, in_bytes) != DCTZHIP_OK) die("H2D (batch)");
  if (dctzhip_decompress_batch(c, k, items, DCTZ_MODE, NULL) != DCTZHIP_OK) die("dctzhip_decompress_batch");
  if (dctzhip_memcpy_d2h(c, hp + in_bytes, dp + in_bytes, total - in_bytes) != DCTZHIP_OK) die("D2H (batch)");
  for (int i = 0; i < k; i++) memcpy(var_bytes(vars_r[i]), hp + off_out[i], vs[i].n * vs[i].ts);
  free(vs); free(off_bin); free(items); free(jobs); free(qtabs);
  return 1;
}

/* ------------------------------------------------------- container check --- */
/* dctz_decompress() trusts the header the way the reference does (dctz-decomp-lib.c:84-100:
 * no size is checked against the buffer, a corrupt file reads out of bounds).  A caller that
 * knows how many bytes it holds runs this first: it checks the layout of dctz-comp-lib.c:775-820
 * against `zbytes`, the plausibility of the header fields, and -- deep != 0 -- that the three
 * sections really inflate to N, 4*nblk and 4*cnt bytes (no GPU involved). */
int dctz_check_container(const void *z, size_t zbytes, int max_elements, int deep) {
  if (!z || zbytes < DZC_HEADER_BYTES) return DCTZ_CHECK_TRUNCATED;
  dzc_view v;
  dzc_header(&v, z, DCTZ_QT, DZC_TYPE_IN_HEADER);
  if ((v.base != FLOAT && v.base != DOUBLE) || ((unsigned)v.h.datatype >> 16) || (v.nd != 0 && v.nd != 2 && v.nd != 3)) return DCTZ_CHECK_BAD_HEADER;
  if (v.n == 0 || v.n > 0x7FFFFFFFu) return DCTZ_CHECK_BAD_HEADER;                             /* N is an int, dctz.h:126 */
  if (max_elements > 0 && v.n > (unsigned int)max_elements) return DCTZ_CHECK_TOO_LARGE;
  if (!(v.h.error_bound >= 1E-6) || v.h.error_bound != v.h.error_bound) return DCTZ_CHECK_BAD_HEADER;   /* :135-138 */
  if (v.nd) {                                           /* multi-dimensional blocks: the extents follow the last section */
    if (zbytes < v.ix_off) return DCTZ_CHECK_TRUNCATED;
    if (dzc_geometry(&v) != 0 || (v.nd == 2 && v.dims[2] != 0)) return DCTZ_CHECK_BAD_HEADER;
  }
  if ((size_t)v.cnt > v.npos - v.nblk) return DCTZ_CHECK_BAD_HEADER;                            /* at most 63 per block */
  if (v.qtable && v.bindex_count != v.npos) return DCTZ_CHECK_BAD_HEADER;                       /* :798 */
  if (zbytes < v.ix_off) return DCTZ_CHECK_TRUNCATED;
  /* Sections that carry the mark of the GPU entropy stage (78 5E): dctz_decompress will look for the "DZIX" chunk index
   * BEHIND the container -- it has no size to check that against, this function has.  The index must be there in full
   * and describe the sections exactly (the same test as the reader's), or the container is refused: a foreign stream
   * that merely starts 78 5E (zlib at levels 2 .. 5 writes those bytes too) would make the reader look past the buffer. */
  uint32_t *sizes[3];
  size_t chunk = 0;
  const int ix = dzc_read_index(&v, zbytes, &chunk, sizes);
  for (int i = 0; i < 3; i++) free(sizes[i]);
  if (ix == DZC_IX_CUT) return DCTZ_CHECK_TRUNCATED;
  if (ix == DZC_IX_BAD) return DCTZ_CHECK_BAD_STREAM;
  if (!deep) return DCTZ_CHECK_OK;
  for (int i = 0; i < 3; i++) {
    /* inflate into a small window, counting: the section must end exactly at `raw[i]` bytes */
    z_stream st;
    unsigned char win[65536];
    memset(&st, 0, sizeof(st));
    if (inflateInit(&st) != Z_OK) return DCTZ_CHECK_BAD_STREAM;
    st.next_in = (Bytef *)v.sec[i]; st.avail_in = v.zlen[i];
    size_t produced = 0;
    int rc;
    do {
      st.next_out = win; st.avail_out = sizeof(win);
      rc = inflate(&st, Z_NO_FLUSH);
      produced += sizeof(win) - st.avail_out;
    } while (rc == Z_OK && produced <= v.raw[i]);
    inflateEnd(&st);
    if (rc != Z_STREAM_END || produced != v.raw[i]) return DCTZ_CHECK_BAD_STREAM;
  }
  return DCTZ_CHECK_OK;
}

/* ------------------------------------------------------------ decompress --- */
/* ---- dctz_decompress, pipelined (round 4) ------------------------------------------------------------------------------
 * A container whose sections are independent chunks ("DZIX") is rebuilt GROUP by group of DCTZ_PIPE_GROUP elements
 * (default 8 Mi): while the host threads inflate the chunks of the groups ahead, the streams of the groups that are
 * complete go to the device, their blocks are rebuilt there (dctzhip_decompress on the group's slices: a group is a
 * range of whole blocks, and its first "stored exactly" coefficient is the number of flags in front of it -- the running
 * `pos` of dctz-decomp-lib.c:402-412 -- which the inflating threads count on the way), and a copier thread brings finished
 * groups back into the caller's array.  Round 3 ran inflate (17 ms per GiB), H2D (3), kernels (0.3) and D2H (21) one after
 * the other; the stages now overlap and the call takes about as long as its longest one.  The reconstruction is the same
 * bytes: the same kernels on the same inputs.  DCTZ_PIPELINE=0: the serial path. */
typedef struct {
  const unsigned char *src;
  unsigned int zlen, len;
  unsigned char *dst;
  uLong adler;
  unsigned int n255;          /* bytes == 255 in the chunk (bin_index chunks: flags + block heads) */
  int count255;
  volatile int done;          /* 1: inflated, 2: does not inflate */
} pp_chunk;
typedef struct {
  pp_chunk *chunks;
  size_t nchunks;
  size_t next;
} pp_queue;
static void pp_do(pp_chunk *c) {
  z_stream zs;
  int bad = 0;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, -15) != Z_OK) bad = 1;
  else {
    zs.next_in = (Bytef *)c->src; zs.avail_in = c->zlen;
    zs.next_out = c->dst; zs.avail_out = c->len;
    const int rc = inflate(&zs, Z_SYNC_FLUSH);
    if ((rc != Z_OK && rc != Z_BUF_ERROR) || zs.avail_in != 0 || zs.avail_out != 0) bad = 1;
    inflateEnd(&zs);
  }
  if (!bad) {
    c->adler = adler32(adler32(0L, Z_NULL, 0), c->dst, c->len);
    if (c->count255) {
      unsigned int k = 0;
      for (unsigned int i = 0; i < c->len; i++) k += (c->dst[i] == 255);
      c->n255 = k;
    }
  }
  __atomic_store_n(&c->done, bad ? 2 : 1, __ATOMIC_RELEASE);
}
static int pp_step(pp_queue *q) {                       /* one chunk, if any is left; 0: the list is exhausted */
  const size_t i = __atomic_fetch_add(&q->next, 1, __ATOMIC_RELAXED);
  if (i >= q->nchunks) return 0;
  pp_do(&q->chunks[i]);
  return 1;
}
static void *pp_worker(void *arg) {
  while (pp_step((pp_queue *)arg)) {}
  return NULL;
}
/* returns 1: done; 0: not applicable / something does not inflate -- the caller takes the serial path (and its way of
 * reporting damage) */
static int decompress_pipelined(dctzhip_ctx *c, const dzc_view *v, size_t chunk, uint32_t *const sizes[3], t_var *var_r, size_t *got_out) {
  const size_t ts = v->ts, n = v->n, cnt = v->cnt;
  const int dtype = v->is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const unsigned char *const *sec = v->sec;
  const size_t *raw = v->raw;
  double qbuf[BLK_SZ];
  const void *qtable = dzc_qtable(v, qbuf);               /* :193-199 */
  const size_t gel = pipe_group();
  if (gel % (16 * chunk) != 0 || n < 2 * gel) return 0;
  const size_t G = (n + gel - 1) / gel;
  if (G > DCTZHIP_D2H_PIPE_MAX_MARKS) return 0;           /* (more groups than the D2H pipe has marks -> the serial path) */
  size_t nch[3], total = 0;
  for (int i = 0; i < 3; i++) { nch[i] = (raw[i] + chunk - 1) / chunk; total += nch[i]; }
  unsigned char *const dst[3] = {(unsigned char *)host_buf(0, raw[0]), (unsigned char *)host_buf(1, raw[1]), (unsigned char *)host_buf(2, raw[2])};
  pp_chunk *chunks = (pp_chunk *)calloc(total ? total : 1, sizeof(pp_chunk));
  size_t *first[3];                                     /* position of a section's chunk j in the (priority-ordered) list */
  for (int i = 0; i < 3; i++) first[i] = (size_t *)malloc((nch[i] ? nch[i] : 1) * sizeof(size_t));
  size_t *goff = (size_t *)malloc(G * sizeof(size_t)), *gbytes = (size_t *)malloc(G * sizeof(size_t));
  if (!chunks || !first[0] || !first[1] || !first[2] || !goff || !gbytes) { fprintf(stderr, "Out of memory: chunk list\n"); exit(1); }
  /* the list in the order the groups need it: group g's bin_index and DC chunks, and the g-th share of AC_exact's */
  size_t zoff[3] = {2, 2, 2}, nextc[3] = {0, 0, 0}, k = 0;
  const size_t bpg = gel / chunk, dpg = gel / 16 / chunk;
  for (size_t g = 0; g < G; g++) {
    const size_t upto[3] = {(g + 1) * bpg < nch[0] ? (g + 1) * bpg : nch[0], (g + 1) * dpg < nch[1] ? (g + 1) * dpg : nch[1],
                            g + 1 == G ? nch[2] : nch[2] * (g + 1) / G};
    for (int i = 0; i < 3; i++)
      for (; nextc[i] < upto[i]; nextc[i]++, k++) {
        const size_t j = nextc[i];
        chunks[k].src = sec[i] + zoff[i]; chunks[k].zlen = sizes[i][j];
        chunks[k].dst = dst[i] + j * chunk;
        chunks[k].len = (unsigned int)(raw[i] - j * chunk < chunk ? raw[i] - j * chunk : chunk);
        chunks[k].count255 = (i == 0);
        zoff[i] += sizes[i][j];
        first[i][j] = k;
      }
  }
  pp_queue q = {chunks, total, 0};
  int threads = host_threads();
  if ((size_t)threads > total) threads = total ? (int)total : 1;
  pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)threads);
  int started = 0;
  if (th) for (int t = 0; t < threads; t++) { if (pthread_create(&th[started], NULL, pp_worker, &q)) break; started++; }

  grow(&g_dev.out, &g_dev.out_cap, n * ts);
  if (dctzhip_d2h_pipe_begin(c, var_bytes(var_r), g_dev.out, n * ts) != DCTZHIP_OK) die("D2H pipe");
  int ok = 1;
  size_t S = 0, ac_up = 0;                               /* exact coefficients consumed so far; bytes of AC_exact on the device */
  const int dbg = getenv("DCTZ_PIPE_DEBUG") != NULL;
  const double tp0 = now_s();
  for (size_t g = 0; g < G && ok; g++) {
    const double tg0 = now_s();
    const size_t e0 = g * gel, ne = n - e0 < gel ? n - e0 : gel;
    const size_t b0 = e0 / BLK_SZ, nb = CEIL(ne, BLK_SZ);
    /* wait for the group's bin_index and DC chunks (helping with whatever chunk is next meanwhile) */
    size_t flags = 0;
    const size_t c_lo[2] = {e0 / chunk, b0 * sizeof(float) / chunk};
    const size_t c_hi[2] = {(e0 + ne + chunk - 1) / chunk, ((b0 + nb) * sizeof(float) + chunk - 1) / chunk};
    for (int i = 0; i < 2 && ok; i++)
      for (size_t j = c_lo[i]; j < c_hi[i] && ok; j++) {
        pp_chunk *pc = &chunks[first[i][j]];
        int d;
        while ((d = __atomic_load_n(&pc->done, __ATOMIC_ACQUIRE)) == 0) { if (!pp_step(&q)) sched_yield(); }
        if (d != 1) ok = 0;
        if (i == 0) flags += pc->n255;
      }
    if (!ok) break;
    /* every block's first byte is the 255 of dctz-comp-lib.c:361, not a flag -- in a container this library or the reference
     * wrote.  One whose block heads are something else (adler-valid all the same) would make the count wrap and the groups'
     * places in AC_exact go backwards while the kernels, which never look at byte 0, rebuild something else than the serial
     * path does: such a container takes the serial path. */
    if (flags < nb) { ok = 0; break; }
    flags -= nb;
    size_t S1 = S + flags;
    if (S1 > cnt) S1 = cnt;                                /* (a stream that flags more than it brings: the kernels report it) */
    for (size_t j = ac_up / chunk; j < (S1 * sizeof(float) + chunk - 1) / chunk && ok; j++) {
      pp_chunk *pc = &chunks[first[2][j]];
      int d;
      while ((d = __atomic_load_n(&pc->done, __ATOMIC_ACQUIRE)) == 0) { if (!pp_step(&q)) sched_yield(); }
      if (d != 1) ok = 0;
    }
    if (!ok) break;
    const double tg1 = now_s();
    /* the group's streams -> device */
    if (dctzhip_memcpy_h2d(c, (unsigned char *)g_dev.bin + e0, dst[0] + e0, ne) != DCTZHIP_OK) die("H2D bin_index");
    if (dctzhip_memcpy_h2d(c, (unsigned char *)g_dev.dc + b0 * sizeof(float), dst[1] + b0 * sizeof(float), nb * sizeof(float)) != DCTZHIP_OK) die("H2D DC");
    const size_t ac_to = S1 * sizeof(float);
    if (ac_to > ac_up) {
      if (dctzhip_memcpy_h2d(c, (unsigned char *)g_dev.ac + ac_up, dst[2] + ac_up, ac_to - ac_up) != DCTZHIP_OK) die("H2D AC_exact");
      ac_up = ac_to;
    }
    const double tg2 = now_s();
    if (dctzhip_decompress(c, (unsigned char *)g_dev.bin + e0, (const float *)g_dev.dc + b0, (const float *)g_dev.ac + S, (uint32_t)(cnt - S), qtable, ne, dtype,
                           v->h.error_bound, v->sf, DCTZ_MODE, (unsigned char *)g_dev.out + e0 * ts) != DCTZHIP_OK) die("dctzhip_decompress");
    if (dbg) fprintf(stderr, "[pipe] group %zu: start %.2f ms, waited %.2f for its chunks, H2D %.2f, call %.2f\n", g, (tg0 - tp0) * 1e3, (tg1 - tg0) * 1e3, (tg2 - tg1) * 1e3, (now_s() - tg2) * 1e3);
    S = S1;
    if (dctzhip_d2h_pipe_advance(c, (e0 + ne) * ts) != DCTZHIP_OK) die("D2H pipe");     /* the group's bytes: complete behind its kernels */
  }
  while (pp_step(&q)) {}                                   /* (what is left of the list: chunks no group waited for) */
  for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
  if (dbg) fprintf(stderr, "[pipe] all groups queued at %.2f ms\n", (now_s() - tp0) * 1e3);
  if (dctzhip_d2h_pipe_end(c, !ok) != DCTZHIP_OK) die("D2H output");
  if (dbg) fprintf(stderr, "[pipe] copies done at %.2f ms\n", (now_s() - tp0) * 1e3);
  /* what inflate() checks at the end of a stream: the adler32 of the content */
  for (int i = 0; i < 3 && ok; i++) {
    uLong a = adler32(0L, Z_NULL, 0);
    for (size_t j = 0; j < nch[i]; j++) { const pp_chunk *pc = &chunks[first[i][j]]; if (pc->done != 1) ok = 0; a = adler32_combine(a, pc->adler, (z_off_t)pc->len); }
    if (a != get_be32(sec[i] + v->zlen[i] - 4)) ok = 0;
  }
  free(th); free(chunks); free(goff); free(gbytes);
  for (int i = 0; i < 3; i++) free(first[i]);
  if (!ok) fprintf(stderr, "libdctz: a chunk of an indexed section does not inflate; falling back to the one-stream inflate\n");
  *got_out = n;
  return ok;
}

/* dctzhip_fixup_apply or dctzhip_fixup_apply_nd, as the container says: the list `a` over the whole array in g_dev.out */
static int fixup_apply_dev(dctzhip_ctx *c, const dzc_view *v, dzfx_arrays a, uint32_t count) {
  const int dtype = v->is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const size_t whole[1] = {v->n}, zero[3] = {0, 0, 0};
  return v->nd ? dctzhip_fixup_apply_nd(c, a.start, a.off, a.val, count, v->nd, v->dims, dtype, zero, v->dims, g_dev.out)
               : dctzhip_fixup_apply(c, a.start, a.off, a.val, count, v->n, dtype, 1, whole, zero, whole, g_dev.out);
}

/* fix (or NULL): a checked correction-list blob of this container (dctz_decompress_bounded), applied to the reconstruction on
 * the device before it is copied back; -1 if the list contradicts itself. */
/* fix (or NULL): a checked correction-list blob, applied to the reconstruction; mask_words (or NULL): the words of a
 * missing-value mask, whose set bits then receive `fill` -- in that order (include/dctz_hip.h, "composed guarantee") */
static int decompress_whole(t_var *var_z, t_var *var_r, const unsigned char *fix, const uint64_t *mask_words, double fill) {
  const double t_begin = now_s();
  dzc_view v;
  const int bad_nd = dzc_open(&v, var_z, DCTZ_QT); /* dctz-decomp-lib.c:84-94 */
  const int is_d = v.is_d, nd = v.nd;
  const size_t ts = v.ts, n = v.n, nblk = v.nblk, npos = v.npos;
  const int dtype = is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const unsigned int cnt = v.cnt;
  if (n == 0) { fprintf(stderr, "libdctz: empty stream\n"); exit(1); }
  /* multi-dimensional blocks (dctz.h: dctz_set_block_dims): the extents sit behind the last section */
  if (bad_nd) { fprintf(stderr, "libdctz: bad multi-dimensional container\n"); exit(1); }

  double t0 = now_s();
  dctzhip_ctx *c = ctx();
  /* sections written by the GPU entropy stage start 78 5E and bring a chunk index: only then are the bytes behind the
   * container looked at.  On request (DCTZ_INFLATE_GPU=1) they are inflated on the device, one lane per chunk -- the
   * compressed sections go over PCIe instead of the raw streams, no host core inflates (include/dctz_hip.h:
   * dctzhip_inflate); otherwise by host threads, chunks side by side. */
  uint32_t *ix_sizes[3] = {NULL, NULL, NULL};
  size_t ix_chunk_bytes = 0;
  const int indexed = dzc_read_index(&v, DZC_UNKNOWN, &ix_chunk_bytes, ix_sizes) == DZC_IX_OK;
  int on_device = 0;
  double t_h2d_z = 0.0;
  grow(&g_dev.bin, &g_dev.bin_cap, npos);
  grow(&g_dev.dc, &g_dev.dc_cap, nblk * sizeof(float));
  grow(&g_dev.ac, &g_dev.ac_cap, (cnt ? cnt : 4) * sizeof(float));
  if (indexed && !nd && !inflate_gpu() && pipeline_on() && !fix && !mask_words) {
    size_t got_p = 0;
    if (decompress_pipelined(c, &v, ix_chunk_bytes, ix_sizes, var_r, &got_p)) {
      for (int i = 0; i < 3; i++) free(ix_sizes[i]);
      if (!quiet()) printf("uncompressed bin_index size is: %lu\n", (unsigned long)got_p); /* :260-262 */
      g_times.zlib_s = 0.0; g_times.h2d_s = 0.0; g_times.gpu_s = 0.0; g_times.d2h_s = 0.0;   /* (the stages overlap: only the total means something) */
      g_times.total_s = now_s() - t_begin;
      return 1;
    }
  }
  if (indexed && inflate_gpu() && ix_chunk_bytes == dctzhip_deflate_chunk_bytes()) {
    size_t zlen[3];
    for (int i = 0; i < 3; i++) {
      zlen[i] = v.zlen[i];
      grow(&g_dev.z[i], &g_dev.z_cap[i], v.zlen[i]);
      if (dctzhip_memcpy_h2d(c, g_dev.z[i], v.sec[i], v.zlen[i]) != DCTZHIP_OK) die("H2D compressed section");
    }
    t_h2d_z = now_s() - t0;
    void *const ddst[3] = {g_dev.bin, g_dev.dc, g_dev.ac};
    int ok = 0;
    if (dctzhip_inflate(c, 3, (const void *const *)g_dev.z, zlen, (const uint32_t *const *)ix_sizes, v.raw, ddst, &ok) != DCTZHIP_OK) die("dctzhip_inflate");
    on_device = ok;            /* 0: inconsistent -- the host path below decides, and reports damage like the reference */
  }

  t_bin_id *bin_index = NULL;
  float *DC = NULL, *AC_exact = NULL;
  uLong got = (uLong)npos;
  if (!on_device) {
  bin_index = (t_bin_id *)host_buf(0, npos);
  DC = (float *)host_buf(1, nblk * sizeof(float));
  AC_exact = (float *)host_buf(2, (size_t)cnt * sizeof(float));
  /* three inflates, in order (dctz-decomp-lib.c:244-322) */
  unsigned char *const rawp[3] = {(unsigned char *)bin_index, (unsigned char *)DC, (unsigned char *)AC_exact};
  if (indexed && inflate_indexed(&v, rawp, ix_chunk_bytes, ix_sizes)) {   /* chunks side by side on host threads */
    got = (uLong)npos;
  } else if (zlib_threads() == 0 || zlib_threads() > 3) {   /* the sections are independent streams: inflate them side by side
                                                               (DCTZ_ZLIB_THREADS=1..3 keeps the reference's one-after-the-other) */
    inflate_job ij[3] = {{v.sec[0], v.zlen[0], (uLong)v.raw[0], 0, bin_index}, {v.sec[1], v.zlen[1], (uLong)v.raw[1], 0, DC},
                         {v.sec[2], v.zlen[2], (uLong)v.raw[2], 0, AC_exact}};
    pthread_t th[2];
    int started = 0;
    for (int i = 1; i < 3; i++) { if (pthread_create(&th[started], NULL, inflate_main, &ij[i])) inflate_main(&ij[i]); else started++; }
    inflate_main(&ij[0]);
    for (int i = 0; i < started; i++) pthread_join(th[i], NULL);
    got = ij[0].produced;
  } else {
    got = inflate_into(v.sec[0], v.zlen[0], bin_index, v.raw[0]);
    inflate_into(v.sec[1], v.zlen[1], DC, v.raw[1]);
    inflate_into(v.sec[2], v.zlen[2], AC_exact, v.raw[2]);
  }
  }
  for (int i = 0; i < 3; i++) free(ix_sizes[i]);
  if (!quiet()) printf("uncompressed bin_index size is: %lu\n", got); /* :260-262 */
  double qbuf[BLK_SZ];
  const void *qtable = dzc_qtable(&v, qbuf);             /* :193-199 */
  double t1 = now_s();

  grow(&g_dev.out, &g_dev.out_cap, n * ts);
  if (!on_device) {
    if (dctzhip_memcpy_h2d(c, g_dev.bin, bin_index, npos) != DCTZHIP_OK) die("H2D bin_index");
    if (dctzhip_memcpy_h2d(c, g_dev.dc, DC, nblk * sizeof(float)) != DCTZHIP_OK) die("H2D DC");
    if (cnt && dctzhip_memcpy_h2d(c, g_dev.ac, AC_exact, (size_t)cnt * sizeof(float)) != DCTZHIP_OK) die("H2D AC_exact");
  }
  double t2 = now_s();

  int rc = nd ? dctzhip_decompress_nd(c, g_dev.bin, (const float *)g_dev.dc, (const float *)g_dev.ac, cnt, qtable, nd, v.dims,
                                      dtype, v.h.error_bound, v.sf, DCTZ_MODE, g_dev.out)
              : dctzhip_decompress(c, g_dev.bin, (const float *)g_dev.dc, (const float *)g_dev.ac, cnt, qtable, n, dtype,
                                   v.h.error_bound, v.sf, DCTZ_MODE, g_dev.out);
  if (rc != DCTZHIP_OK) die("dctzhip_decompress");
  if (dctzhip_sync(c) != DCTZHIP_OK) die("sync");   /* (stage timers: the call returns while the reconstruction is being written) */
  if (fix) {
    dzfx_header fh;
    memcpy(&fh, fix, sizeof(fh));
    const size_t payload = dzfx_payload_bytes((size_t)fh.tiles, (size_t)fh.count, ts);
    grow(&g_dev.fix, &g_dev.fix_cap, payload);
    if (dctzhip_memcpy_h2d(c, g_dev.fix, fix + dzfx_header_bytes(fh.version), payload) != DCTZHIP_OK) die("H2D correction list");
    rc = fixup_apply_dev(c, &v, dzfx_arrays_at(g_dev.fix, (size_t)fh.tiles, (size_t)fh.count), (uint32_t)fh.count);
    if (rc == DCTZHIP_E_ARG) return -1;                /* the list contradicts itself or the array: nothing is handed out */
    if (rc != DCTZHIP_OK) die("dctzhip_fixup_apply");
  }
  if (mask_words) {
    const size_t whole[1] = {n}, zero[1] = {0};
    const size_t mbytes = dctzhip_mask_words(n) * sizeof(uint64_t);
    grow(&g_dev.fix, &g_dev.fix_cap, mbytes);
    if (dctzhip_memcpy_h2d(c, g_dev.fix, mask_words, mbytes) != DCTZHIP_OK) die("H2D mask");
    if (dctzhip_mask_apply(c, (const uint64_t *)g_dev.fix, n, dtype, fill, 1, whole, zero, whole, g_dev.out) != DCTZHIP_OK) die("dctzhip_mask_apply");
  }
  double t3 = now_s();
  if (dctzhip_memcpy_d2h(c, var_bytes(var_r), g_dev.out, n * ts) != DCTZHIP_OK) die("D2H output");
  double t4 = now_s();

  g_times.zlib_s = t1 - t0; g_times.h2d_s = t2 - t1; g_times.gpu_s = t3 - t2; g_times.d2h_s = t4 - t3;
  if (on_device) { g_times.zlib_s -= t_h2d_z; g_times.h2d_s += t_h2d_z; }      /* the compressed sections' way to the device is a copy, not inflate */
  g_times.total_s = now_s() - t_begin;
  return 1;
}

/* ------------- dctz_decompress_range, dctz_decompress_box, dctz_decompress_boxes, dctz_decompress_box_nd, dctz_decompress_boxes_nd -- */
/* The first `want` bytes of one section into dst.  Indexed (sizes != NULL): only the chunks that hold them, side by side
 * on host threads (dst has room for whole chunks: min(raw, chunks * chunk) bytes); a chunk that does not inflate sends the
 * section to the streaming inflate.  Otherwise one inflate that stops once `want` bytes are out.  Returns the bytes made. */
static size_t inflate_prefix(const unsigned char *sec, unsigned int zlen, size_t raw, size_t want, unsigned char *dst, size_t chunk,
                             const uint32_t *sizes) {
  if (want == 0) return 0;
  if (sizes) {
    const size_t nch = (want + chunk - 1) / chunk;
    ix_chunk *chunks = (ix_chunk *)calloc(nch, sizeof(ix_chunk));
    if (!chunks) { fprintf(stderr, "Out of memory: chunk list\n"); exit(1); }
    size_t off = 2;
    for (size_t j = 0; j < nch; j++) {
      chunks[j].src = sec + off; chunks[j].zlen = sizes[j];
      chunks[j].dst = dst + j * chunk;
      chunks[j].len = (unsigned int)(raw - j * chunk < chunk ? raw - j * chunk : chunk);
      off += sizes[j];
    }
    ix_run(chunks, nch);
    int ok = 1;
    for (size_t j = 0; j < nch; j++) if (chunks[j].err) ok = 0;
    free(chunks);
    if (ok) return want;
  }
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return 0;
  zs.next_in = (Bytef *)sec;
  zs.avail_in = zlen;
  size_t done = 0;
  while (done < want) {
    const size_t left = want - done;
    const uInt step = left > ((size_t)1 << 30) ? (uInt)1 << 30 : (uInt)left;
    zs.next_out = (Bytef *)dst + done;
    zs.avail_out = step;
    const int rc = inflate(&zs, Z_NO_FLUSH);
    done += step - zs.avail_out;
    if (rc != Z_OK) break;                                   /* end of stream, damage, or no progress */
  }
  inflateEnd(&zs);
  return done;
}

/* The way from a container's sections to the device, for every reader that does not decode the whole array: the first
 * bin_bytes of bin_index and the first dc_bytes of DC inflated and uploaded (DC into room for dc_room >= dc_bytes bytes), the
 * exception index built over those bin ids, and as many AC_exact words as it counts -- idx[t] of a prefix's index is idx[t]
 * of the whole array's.  dc_only: the DC section alone; bin, ac and idx stay NULL and ac_count 0.  Returns 1, or -1 for a
 * section that does not hold its prefix or bin ids that flag more than the header counts, with nothing left to free.  It is
 * the first thing in a reader that asks for the device: every refusal of the arguments comes before it. */
typedef struct {
  dctzhip_ctx *c;
  const void *bin;
  const float *dc, *ac;
  const uint32_t *idx;
  uint32_t ac_count;
  const void *qtable;                                        /* NULL, or qbuf */
  double qbuf[BLK_SZ];
  double t_zlib, t_h2d;                                      /* seconds inflating; seconds copying and indexing */
} dev_streams;
#define DEV_STREAMS(s) (s).c, (s).bin, (s).dc, (s).ac, (s).ac_count, (s).idx, (s).qtable   /* as every dctzhip_ reader takes them */
static int sections_to_device(const dzc_view *v, size_t bin_bytes, size_t dc_bytes, size_t dc_room, int dc_only, dev_streams *s) {
  memset(s, 0, sizeof(*s));
  dctzhip_ctx *c = s->c = ctx();
  uint32_t *ix_sizes[3] = {NULL, NULL, NULL};
  size_t chunk = 0;
  const int indexed = dzc_read_index(v, DZC_UNKNOWN, &chunk, ix_sizes) == DZC_IX_OK;
  s->qtable = dzc_qtable(v, s->qbuf);                        /* :193-199 */
  void **const dp[3] = {&g_dev.bin, &g_dev.dc, &g_dev.ac};
  size_t *const cp[3] = {&g_dev.bin_cap, &g_dev.dc_cap, &g_dev.ac_cap};
  size_t want[3] = {bin_bytes, dc_bytes, 0};                 /* AC_exact: known once the index is built */
  int ret = -1;
  double t0;
  for (int i = 0; i < 3; i++) {
    if (dc_only && i != 1) continue;
    if (i == 2) {
      t0 = now_s();
      grow(&g_dev.idx, &g_dev.idx_cap, dctzhip_ac_index_len(bin_bytes) * sizeof(uint32_t));
      if (dctzhip_ac_index(c, g_dev.bin, bin_bytes, (uint32_t *)g_dev.idx, &s->ac_count) != DCTZHIP_OK) die("dctzhip_ac_index");
      if (s->ac_count > v->cnt) goto out;                    /* the bin ids flag more than the header counts */
      want[2] = (size_t)s->ac_count * sizeof(float);
      s->t_h2d += now_s() - t0;
    }
    t0 = now_s();
    const size_t room = indexed ? MIN(v->raw[i], (want[i] + chunk - 1) / chunk * chunk) : want[i];
    unsigned char *hp = (unsigned char *)host_buf(i, room);
    if (inflate_prefix(v->sec[i], v->zlen[i], v->raw[i], want[i], hp, chunk, indexed ? ix_sizes[i] : NULL) < want[i]) goto out;
    s->t_zlib += now_s() - t0;
    t0 = now_s();
    const size_t dev = i == 1 ? dc_room : want[i];
    grow(dp[i], cp[i], dev ? dev : 4);
    if (want[i] && dctzhip_memcpy_h2d(c, *dp[i], hp, want[i]) != DCTZHIP_OK) die("H2D section");
    s->t_h2d += now_s() - t0;
  }
  s->dc = (const float *)g_dev.dc;
  if (!dc_only) { s->bin = g_dev.bin; s->ac = (const float *)g_dev.ac; s->idx = (const uint32_t *)g_dev.idx; }
  ret = 1;
out:
  for (int i = 0; i < 3; i++) free(ix_sizes[i]);
  return ret;
}
/* The stage times of such a reader: the loader's (with what the reader added of its own), the device calls from t_gpu to
 * t_d2h, the copy back from there to now. */
static void part_times(const dev_streams *s, double t_begin, double t_gpu, double t_d2h) {
  g_times.zlib_s = s->t_zlib; g_times.h2d_s = s->t_h2d; g_times.gpu_s = t_d2h - t_gpu; g_times.d2h_s = now_s() - t_d2h;
  g_times.total_s = now_s() - t_begin;
}

/* dctz_decompress_range (ndim == 0: elements [lo, hi)), dctz_decompress_box (ndim >= 1: the box; [lo, hi) becomes
 * [first box element, last box element + 1)) and dctz_decompress_box_nd (ndim == PART_TILED: a DZND container, geometry and
 * extents from the container; [lo, hi) becomes the stream positions [64 * first intersecting block, 64 * (last + 1))): the
 * prefix of the sections that span needs, its index, one device call, and only the wanted elements copied back. */
#define PART_TILED (-1)
/* dctz_decompress_boxes: k boxes (rows of ndim entries) of one container through the same machinery ONCE -- the prefix of
 * the sections up to the last element of any box, one index, one dctzhip_decompress_boxes into one device arena, k copies
 * back.  dctz_decompress_boxes_nd (PART_TILED with a list): the same for a DZND container, rows of the container's own
 * number of dimensions, the span from 64 * the first intersecting block of any box to 64 * (the last of any + 1), one
 * dctzhip_decompress_boxes_nd. */
typedef struct { int k; const size_t *lo, *hi; t_var *const *var_r; } part_list;
/* A box against n elements seen as dims: 0 and its first and last flat element and its element count, or -1. */
static int box_span(size_t n, int ndim, const size_t *dims, const size_t *blo, const size_t *bhi, size_t *first, size_t *last, size_t *elems) {
  if (ndim < 1 || ndim > DCTZHIP_BOX_MAXDIM || !dims || !blo || !bhi || n == 0) return -1;
  size_t prod = 1;
  *first = 0; *last = 0; *elems = 1;
  for (int i = 0; i < ndim; i++) {
    if (dims[i] == 0 || dims[i] > n / prod || blo[i] >= bhi[i] || bhi[i] > dims[i]) return -1;
    prod *= dims[i];
    *elems *= bhi[i] - blo[i];
    *first = *first * dims[i] + blo[i];
    *last = *last * dims[i] + (bhi[i] - 1);
  }
  return prod == n ? 0 : -1;
}
/* A box against the extents of a DZND container: 0 and its first and last intersecting block of the row-major block grid and
 * its element count, or -1. */
static int tiled_span(const dzc_view *v, const size_t *blo, const size_t *bhi, size_t *first, size_t *last, size_t *elems) {
  if (!blo || !bhi) return -1;
  const size_t edge = v->nd == 2 ? 8 : 4;
  *first = 0; *last = 0; *elems = 1;
  for (int i = 0; i < v->nd; i++) {
    if (blo[i] >= bhi[i] || bhi[i] > v->dims[i]) return -1;
    const size_t nb = (v->dims[i] + edge - 1) / edge;
    *elems *= bhi[i] - blo[i];
    *first = *first * nb + blo[i] / edge;
    *last = *last * nb + (bhi[i] - 1) / edge;
  }
  return 0;
}
static int decompress_part(t_var *var_z, size_t lo, size_t hi, int ndim, const size_t *dims, const size_t *blo, const size_t *bhi, t_var *var_r,
                           const part_list *list) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  const int tiled = ndim == PART_TILED;
  if (tiled && (v.nd == 0 || dzc_geometry(&v) != 0)) return -1;    /* a flat container, or extents that are no shape */
  if (!tiled && v.nd != 0) return -1;                              /* DZND: element order is not block order */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk;               /* n: positions of the streams (flat: the elements) */
  const int dtype = v.is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  size_t out_elems;
  dctzhip_box_item *items = NULL;
  const int rows = tiled ? v.nd : ndim;                        /* entries per row of a list's lo / hi */
  if (tiled && n == 0) return -1;
  if (list) {                                                  /* [lo, hi): from the first position of any box to the last of any */
    if (list->k < 1 || list->k > DCTZHIP_BOXES_MAX || !list->lo || !list->hi || !list->var_r) return -1;
    items = (dctzhip_box_item *)calloc((size_t)list->k, sizeof(dctzhip_box_item));
    if (!items) { fprintf(stderr, "Out of memory: box list\n"); exit(1); }
    out_elems = 0;                                             /* the arena: every output at a multiple of 16 bytes */
    for (int j = 0; j < list->k; j++) {
      size_t first, last, elems;
      const size_t *jlo = list->lo + (size_t)j * rows, *jhi = list->hi + (size_t)j * rows;
      if (!list->var_r[j] || (tiled ? tiled_span(&v, jlo, jhi, &first, &last, &elems) : box_span(n, ndim, dims, jlo, jhi, &first, &last, &elems)) != 0) {
        free(items);
        return -1;
      }
      if (tiled) { first *= BLK_SZ; last = (last + 1) * BLK_SZ - 1; }   /* blocks -> stream positions */
      if (j == 0 || first < lo) lo = first;
      if (j == 0 || last + 1 > hi) hi = last + 1;
      for (int i = 0; i < rows; i++) { items[j].lo[i] = jlo[i]; items[j].hi[i] = jhi[i]; }
      items[j].d_out = (void *)(uintptr_t)(out_elems * ts);    /* offset for now: the arena may still move */
      out_elems += (elems * ts + 15) / 16 * 16 / ts;
    }
  } else if (tiled) {
    size_t first, last;
    if (tiled_span(&v, blo, bhi, &first, &last, &out_elems) != 0) return -1;
    lo = first * BLK_SZ; hi = (last + 1) * BLK_SZ;
  } else if (ndim != 0) {
    size_t last;
    if (box_span(n, ndim, dims, blo, bhi, &lo, &last, &out_elems) != 0) return -1;
    hi = last + 1;
  } else {
    out_elems = hi - lo;
  }
  if (n == 0 || lo >= hi || hi > n) { free(items); return -1; }
  const size_t S = DCTZHIP_INDEX_STRIDE;
  const size_t t1 = (hi + S - 1) / S;                        /* the range's tiles end here */
  const size_t dc_dev = MIN(nblk, t1 * (S / BLK_SZ));        /* DC words the range's tiles cover on the device */
  dev_streams s;
  /* bin ids up to the end of the range's tiles (the flags in front give AC_exact's position), DC up to the range's last block */
  if (sections_to_device(&v, MIN(n, S * t1), (hi + BLK_SZ - 1) / BLK_SZ * sizeof(float), dc_dev * sizeof(float), 0, &s) != 1) { free(items); return -1; }
  dctzhip_ctx *c = s.c;
  int ret = -1;
  const double t0 = now_s();
  grow(&g_dev.out, &g_dev.out_cap, out_elems * ts);
  if (list) for (int j = 0; j < list->k; j++) items[j].d_out = (unsigned char *)g_dev.out + (uintptr_t)items[j].d_out;
  const int rc = list && tiled ? dctzhip_decompress_boxes_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, list->k, items)
                 : list    ? dctzhip_decompress_boxes(DEV_STREAMS(s), n, dtype, v.h.error_bound, v.sf, DCTZ_MODE, ndim, dims, list->k, items)
                 : tiled   ? dctzhip_decompress_box_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, blo, bhi, g_dev.out)
                 : ndim == 0 ? dctzhip_decompress_range(DEV_STREAMS(s), n, dtype, v.h.error_bound, v.sf, DCTZ_MODE, lo, hi, g_dev.out)
                           : dctzhip_decompress_box(DEV_STREAMS(s), n, dtype, v.h.error_bound, v.sf, DCTZ_MODE, ndim, dims, blo, bhi, g_dev.out);
  if (rc == DCTZHIP_E_ARG) goto out;                         /* the streams disagree with each other */
  if (rc != DCTZHIP_OK)
    die(list && tiled ? "dctzhip_decompress_boxes_nd" : list ? "dctzhip_decompress_boxes" : tiled ? "dctzhip_decompress_box_nd" : ndim == 0 ? "dctzhip_decompress_range" : "dctzhip_decompress_box");
  const double t1s = now_s();
  if (list) {
    for (int j = 0; j < list->k; j++) {
      size_t elems = 1;
      for (int i = 0; i < rows; i++) elems *= items[j].hi[i] - items[j].lo[i];
      if (dctzhip_memcpy_d2h(c, var_bytes(list->var_r[j]), items[j].d_out, elems * ts) != DCTZHIP_OK) die("D2H output");
    }
  } else if (dctzhip_memcpy_d2h(c, var_bytes(var_r), g_dev.out, out_elems * ts) != DCTZHIP_OK) die("D2H output");
  part_times(&s, t_begin, t0, t1s);
  ret = 1;
out:
  free(items);
  return ret;
}

int dctz_decompress_range(t_var *var_z, size_t lo, size_t hi, t_var *var_r) { return decompress_part(var_z, lo, hi, 0, NULL, NULL, NULL, var_r, NULL); }

int dctz_decompress_box(t_var *var_z, int ndim, const size_t *dims, const size_t *lo, const size_t *hi, t_var *var_r) {
  if (ndim < 1) return -1;
  return decompress_part(var_z, 0, 0, ndim, dims, lo, hi, var_r, NULL);
}

int dctz_decompress_boxes(t_var *var_z, int ndim, const size_t *dims, int k, const size_t *lo, const size_t *hi, t_var *const *var_r) {
  if (ndim < 1 || ndim > DCTZHIP_BOX_MAXDIM) return -1;
  const part_list list = {k, lo, hi, var_r};
  return decompress_part(var_z, 0, 0, ndim, dims, NULL, NULL, NULL, &list);
}

int dctz_decompress_box_nd(t_var *var_z, const size_t *lo, const size_t *hi, t_var *var_r) {
  return decompress_part(var_z, 0, 0, PART_TILED, NULL, lo, hi, var_r, NULL);
}

int dctz_decompress_boxes_nd(t_var *var_z, int k, const size_t *lo, const size_t *hi, t_var *const *var_r) {
  const part_list list = {k, lo, hi, var_r};
  return decompress_part(var_z, 0, 0, PART_TILED, NULL, NULL, NULL, NULL, &list);
}

/* ------------------------------------------------------------- dctz_decompress_coarse -- */
/* The whole array at 1 / factor of its resolution (include/dctz_hip.h: dctzhip_decompress_coarse / _coarse_nd), flat and
 * DZND containers alike: the trailer decides.  With factor == block edge (and no short block) the DC section alone is
 * inflated and uploaded; otherwise the three sections, and the exception index is built once.  Only the coarse array is
 * copied back.  Returns as dctz_decompress_box does: 1, or -1 for a bad factor or streams that disagree with each other. */
int dctz_decompress_coarse(t_var *var_z, int factor, t_var *var_r) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  const int tiled = v.nd != 0;
  if (tiled && dzc_geometry(&v) != 0) return -1;                   /* extents that are no shape */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk;               /* n: positions of the streams (flat: the elements) */
  const int dtype = v.is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const int edge = !tiled ? BLK_SZ : v.nd == 2 ? 8 : 4;
  if (n == 0 || !var_r || factor < 2 || factor > edge || (factor & (factor - 1))) return -1;
  size_t out_elems = 1;
  if (tiled) for (int i = 0; i < v.nd; i++) out_elems *= (v.dims[i] + (size_t)factor - 1) / (size_t)factor;
  else out_elems = dctzhip_coarse_len(n, factor);
  const int dc_only = factor == edge && (tiled || n % BLK_SZ == 0);

  dev_streams s;
  if (sections_to_device(&v, n, nblk * sizeof(float), nblk * sizeof(float), dc_only, &s) != 1) return -1;
  const double t0 = now_s();
  grow(&g_dev.out, &g_dev.out_cap, out_elems * ts);
  const int rc = tiled ? dctzhip_decompress_coarse_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, factor, g_dev.out)
                       : dctzhip_decompress_coarse(DEV_STREAMS(s), n, dtype, v.h.error_bound, v.sf, DCTZ_MODE, factor, g_dev.out);
  if (rc == DCTZHIP_E_ARG) return -1;                        /* the streams disagree with each other */
  if (rc != DCTZHIP_OK) die(tiled ? "dctzhip_decompress_coarse_nd" : "dctzhip_decompress_coarse");
  const double t1s = now_s();
  if (dctzhip_memcpy_d2h(s.c, var_bytes(var_r), g_dev.out, out_elems * ts) != DCTZHIP_OK) die("D2H output");
  part_times(&s, t_begin, t0, t1s);
  return 1;
}

/* ------------------------------------------------------ dctz_decompress_coarse_box_nd -- */
/* A box, in coarse coordinates, of what dctz_decompress_coarse returns for a DZND container (include/dctz_hip.h:
 * dctzhip_decompress_coarse_box_nd), the way of decompress_part: with K = edge / factor the blocks lo / K ... (hi - 1) / K hold
 * the box; bin ids up to the end of the last of their stream tiles, DC up to the last of them -- with factor == edge that
 * DC prefix alone -- the index built once over the prefix, one device call, only the box copied back. */
/* A box in coarse coordinates against the extents of a DZND container (factor is one of the geometry's): 0 and its first and
 * last block of the row-major block grid and its cell count, or -1. */
static int coarse_span(const dzc_view *v, int factor, const size_t *lo, const size_t *hi, size_t *first, size_t *last, size_t *elems) {
  if (!lo || !hi) return -1;
  const size_t edge = v->nd == 2 ? 8 : 4, K = edge / (size_t)factor;
  *first = 0; *last = 0; *elems = 1;
  for (int i = 0; i < v->nd; i++) {
    const size_t cd = (v->dims[i] + (size_t)factor - 1) / (size_t)factor, nb = (v->dims[i] + edge - 1) / edge;
    if (lo[i] >= hi[i] || hi[i] > cd) return -1;
    *elems *= hi[i] - lo[i];
    *first = *first * nb + lo[i] / K;
    *last = *last * nb + (hi[i] - 1) / K;
  }
  return *last >= v->nblk ? -1 : 0;
}
int dctz_decompress_coarse_box_nd(t_var *var_z, int factor, const size_t *lo, const size_t *hi, t_var *var_r) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  if (v.nd == 0 || dzc_geometry(&v) != 0) return -1;               /* a flat container, or extents that are no shape */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk;
  const int dtype = v.is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const int edge = v.nd == 2 ? 8 : 4;
  if (n == 0 || !var_r || !lo || !hi || factor < 2 || factor > edge || (factor & (factor - 1))) return -1;
  const size_t K = (size_t)(edge / factor);
  size_t first = 0, last = 0, out_elems = 1;                   /* blocks of the row-major block grid */
  if (coarse_span(&v, factor, lo, hi, &first, &last, &out_elems) != 0) return -1;
  const int dc_only = K == 1;
  const size_t S = DCTZHIP_INDEX_STRIDE;
  const size_t t1 = ((last + 1) * BLK_SZ + S - 1) / S;         /* the candidate tiles end here */
  const size_t dc_bytes = (last + 1) * sizeof(float);
  const size_t dc_dev = dc_only ? last + 1 : MIN(nblk, t1 * (S / BLK_SZ));   /* DC words the candidate tiles cover on the device */
  dev_streams s;
  if (sections_to_device(&v, dc_only ? 0 : MIN(n, S * t1), dc_bytes, dc_dev * sizeof(float), dc_only, &s) != 1) return -1;
  const double t0 = now_s();
  grow(&g_dev.out, &g_dev.out_cap, out_elems * ts);
  const int rc = dctzhip_decompress_coarse_box_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, factor, lo, hi, g_dev.out);
  if (rc == DCTZHIP_E_ARG) return -1;                          /* the streams disagree with each other */
  if (rc != DCTZHIP_OK) die("dctzhip_decompress_coarse_box_nd");
  const double t1s = now_s();
  if (dctzhip_memcpy_d2h(s.c, var_bytes(var_r), g_dev.out, out_elems * ts) != DCTZHIP_OK) die("D2H output");
  part_times(&s, t_begin, t0, t1s);
  return 1;
}

/* ---------------------------------------------------- dctz_decompress_coarse_boxes_nd -- */
/* k such boxes (rows of the container's own number of dimensions, coarse coordinates, one factor) through the same machinery
 * ONCE (include/dctz_hip.h: dctzhip_decompress_coarse_boxes_nd): bin ids up to the end of the last candidate stream tile of
 * any box and DC up to the last block of any box -- with factor == edge that DC prefix alone -- one index, one device call
 * into one arena (every output at a multiple of 16 bytes), k copies back.  Returns as dctz_decompress_coarse_box_nd does; a bad
 * box anywhere in the list is refused before anything is written. */
int dctz_decompress_coarse_boxes_nd(t_var *var_z, int factor, int k, const size_t *lo, const size_t *hi, t_var *const *var_r) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  if (v.nd == 0 || dzc_geometry(&v) != 0) return -1;               /* a flat container, or extents that are no shape */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk;
  const int dtype = v.is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  const int edge = v.nd == 2 ? 8 : 4;
  if (n == 0 || factor < 2 || factor > edge || (factor & (factor - 1))) return -1;
  if (k < 1 || k > DCTZHIP_BOXES_MAX || !lo || !hi || !var_r) return -1;
  dctzhip_box_item *items = (dctzhip_box_item *)calloc((size_t)k, sizeof(dctzhip_box_item));
  if (!items) { fprintf(stderr, "Out of memory: box list\n"); exit(1); }
  size_t last = 0, out_elems = 0;                              /* the last block of any box; the arena */
  for (int j = 0; j < k; j++) {
    size_t jfirst, jlast, elems;
    const size_t *jlo = lo + (size_t)j * v.nd, *jhi = hi + (size_t)j * v.nd;
    if (!var_r[j] || coarse_span(&v, factor, jlo, jhi, &jfirst, &jlast, &elems) != 0) { free(items); return -1; }
    if (jlast > last) last = jlast;
    for (int i = 0; i < v.nd; i++) { items[j].lo[i] = jlo[i]; items[j].hi[i] = jhi[i]; }
    items[j].d_out = (void *)(uintptr_t)(out_elems * ts);      /* offset for now: the arena may still move */
    out_elems += (elems * ts + 15) / 16 * 16 / ts;
  }
  const int dc_only = factor == edge;
  const size_t S = DCTZHIP_INDEX_STRIDE;
  const size_t t1 = ((last + 1) * BLK_SZ + S - 1) / S;         /* the candidate tiles end here */
  const size_t dc_dev = dc_only ? last + 1 : MIN(nblk, t1 * (S / BLK_SZ));   /* DC words the candidate tiles cover on the device */
  dev_streams s;
  if (sections_to_device(&v, dc_only ? 0 : MIN(n, S * t1), (last + 1) * sizeof(float), dc_dev * sizeof(float), dc_only, &s) != 1) { free(items); return -1; }
  int ret = -1;
  const double t0 = now_s();
  grow(&g_dev.out, &g_dev.out_cap, out_elems * ts);
  for (int j = 0; j < k; j++) items[j].d_out = (unsigned char *)g_dev.out + (uintptr_t)items[j].d_out;
  const int rc = dctzhip_decompress_coarse_boxes_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, factor, k, items);
  if (rc == DCTZHIP_E_ARG) goto out;                           /* the streams disagree with each other */
  if (rc != DCTZHIP_OK) die("dctzhip_decompress_coarse_boxes_nd");
  const double t1s = now_s();
  for (int j = 0; j < k; j++) {
    size_t elems = 1;
    for (int i = 0; i < v.nd; i++) elems *= items[j].hi[i] - items[j].lo[i];
    if (dctzhip_memcpy_d2h(s.c, var_bytes(var_r[j]), items[j].d_out, elems * ts) != DCTZHIP_OK) die("D2H output");
  }
  part_times(&s, t_begin, t0, t1s);
  ret = 1;
out:
  free(items);
  return ret;
}

/* ------------------------------------------------------------------ dctz_tile_summary -- */
/* Per-tile records of the reconstruction, and with var_ref of its error (include/dctz_hip.h: dctzhip_tile_summary,
 * dctzhip_tile_summary_nd): the three sections inflated, the index built once, the original uploaded when given; records and
 * total alone come back.  `tiled`: the container must be a DZND one (geometry and extents from the container, the original
 * is the array in C order), else a flat one -- each entry point refuses the other kind.  Returns as dctz_decompress_box does. */
_Static_assert(sizeof(dctz_tile_summary_t) == sizeof(dctzhip_tile_summary_t), "one record layout");
static int tile_summary_part(t_var *var_z, t_var *var_ref, int N_ref, dctz_tile_summary_t *tiles, dctz_tile_summary_t *total, int tiled) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  if ((v.nd != 0) != (tiled != 0)) return -1;                      /* tiled streams carry edge padding: they need the geometry */
  if (tiled && dzc_geometry(&v) != 0) return -1;                   /* a DZND container whose extents are none */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk, n_ref = v.n;  /* stream positions (tiled: edge padding included); elements */
  const int dtype = v.is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  if (n == 0 || (!tiles && !total)) return -1;
  if (var_ref && ((var_ref->datatype == DOUBLE) != (v.is_d != 0) || N_ref < 0 || (size_t)N_ref != n_ref || !var_bytes(var_ref))) return -1;
  const size_t m = dctzhip_summary_tiles(n);

  dev_streams s;
  if (sections_to_device(&v, n, nblk * sizeof(float), nblk * sizeof(float), 0, &s) != 1) return -1;
  dctzhip_ctx *c = s.c;
  double t0 = now_s();
  if (var_ref) {
    grow(&g_dev.in, &g_dev.in_cap, n_ref * ts);
    if (dctzhip_memcpy_h2d(c, g_dev.in, var_bytes(var_ref), n_ref * ts) != DCTZHIP_OK) die("H2D original");
  }
  if (tiles) grow(&g_dev.out, &g_dev.out_cap, m * sizeof(dctzhip_tile_summary_t));
  s.t_h2d += now_s() - t0;
  t0 = now_s();
  dctzhip_tile_summary_t tot;
  const void *ref = var_ref ? g_dev.in : NULL;
  dctzhip_tile_summary_t *recs = tiles ? (dctzhip_tile_summary_t *)g_dev.out : NULL;
  const int rc = tiled ? dctzhip_tile_summary_nd(DEV_STREAMS(s), v.nd, v.dims, dtype, v.h.error_bound, v.sf, DCTZ_MODE, ref, recs, total ? &tot : NULL)
                       : dctzhip_tile_summary(DEV_STREAMS(s), n, dtype, v.h.error_bound, v.sf, DCTZ_MODE, ref, recs, total ? &tot : NULL);
  if (rc == DCTZHIP_E_ARG) return -1;                        /* the streams disagree with each other */
  if (rc != DCTZHIP_OK) die("dctzhip_tile_summary");
  const double t1s = now_s();
  if (tiles && dctzhip_memcpy_d2h(c, tiles, g_dev.out, m * sizeof(dctzhip_tile_summary_t)) != DCTZHIP_OK) die("D2H records");
  if (total) memcpy(total, &tot, sizeof(tot));
  part_times(&s, t_begin, t0, t1s);
  return 1;
}
int dctz_tile_summary(t_var *var_z, t_var *var_ref, int N_ref, dctz_tile_summary_t *tiles, dctz_tile_summary_t *total) {
  return tile_summary_part(var_z, var_ref, N_ref, tiles, total, 0);
}
int dctz_tile_summary_nd(t_var *var_z, t_var *var_ref, int N_ref, dctz_tile_summary_t *tiles, dctz_tile_summary_t *total) {
  return tile_summary_part(var_z, var_ref, N_ref, tiles, total, 1);
}

/* ------------------------------------------ dctz_fixup_build, dctz_decompress_bounded -- */
int dctz_decompress(t_var *var_z, t_var *var_r) { return decompress_whole(var_z, var_r, NULL, NULL, 0.0); }

/* dctz_decompress with the correction list of `blob` applied (include/dctz.h).  The blob's header is held against the
 * container's before anything else happens. */
int dctz_decompress_bounded(t_var *var_z, const void *blob, size_t blob_bytes, t_var *var_r) {
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype);
  if (v.n == 0 || !var_r) return -1;
  if (v.nd == 0) {
    dzfx_header fh;
    if (dzfx_check(blob, blob_bytes, v.is_d, v.n, &fh) != 0) return -1;
  } else {
    /* a tiled container takes a tiled blob: the blob's version decides before the container's extents are looked at */
    dzfx_header_nd nh;
    if (dzfx_version(blob, blob_bytes) != DZFX_VERSION_ND || dzc_geometry(&v) != 0) return -1;
    if (dzfx_check_nd(blob, blob_bytes, v.is_d, v.nd, v.dims, v.n, v.nblk, &nh) != 0) return -1;
  }
  return decompress_whole(var_z, var_r, (const unsigned char *)blob, NULL, 0.0);
}

/* dctzhip_fixup_build or dctzhip_fixup_build_nd, as the container says: the list of the streams `s` against the original in
 * g_dev.in, into `a` with room for `capacity` entries (a.off and a.val NULL: the tile starts and the count alone) */
static int fixup_build_dev(const dzc_view *v, const dev_streams *s, double bound, dzfx_arrays a, uint32_t capacity, uint32_t *count) {
  const int dtype = v->is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  return v->nd ? dctzhip_fixup_build_nd(DEV_STREAMS(*s), v->nd, v->dims, dtype, v->h.error_bound, v->sf, DCTZ_MODE, g_dev.in, bound, a.start, a.off,
                                        a.val, capacity, count)
               : dctzhip_fixup_build(DEV_STREAMS(*s), v->npos, dtype, v->h.error_bound, v->sf, DCTZ_MODE, g_dev.in, bound, a.start, a.off, a.val,
                                     capacity, count);
}

/* The correction list of a container against the caller's unscaled original, as one malloc'd blob
 * (csrc/dctz_fixup_blob.h): the whole streams to the device (sections_to_device), then a count-only call that sizes the list and the call
 * that fills it.  The container decides: a DZND container gives the list over its stream positions (a version-2 blob), the
 * original being the array in C order. */
int dctz_fixup_build(t_var *var_z, t_var *var_ref, int N_ref, double bound, void **blob, size_t *blob_bytes) {
  const double t_begin = now_s();
  dzc_view v;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype); /* dctz-decomp-lib.c:84-94 */
  const int nd = v.nd;
  if (nd != 0 && dzc_geometry(&v) != 0) return -1;                 /* a DZND container whose extents are none */
  const size_t ts = v.ts, n = v.npos, nblk = v.nblk, n_ref = v.n;  /* stream positions (tiled: edge padding included); elements */
  if (n == 0 || !blob || !blob_bytes || !var_ref || !(bound >= 0.0) || isinf(bound)) return -1;
  if ((var_ref->datatype == DOUBLE) != (v.is_d != 0) || N_ref < 0 || (size_t)N_ref != n_ref || !var_bytes(var_ref)) return -1;
  const size_t m = dctzhip_fixup_tiles(n);

  dev_streams s;
  if (sections_to_device(&v, n, nblk * sizeof(float), nblk * sizeof(float), 0, &s) != 1) return -1;
  dctzhip_ctx *c = s.c;
  double t0 = now_s();
  grow(&g_dev.in, &g_dev.in_cap, n_ref * ts);
  if (dctzhip_memcpy_h2d(c, g_dev.in, var_bytes(var_ref), n_ref * ts) != DCTZHIP_OK) die("H2D original");
  grow(&g_dev.fix, &g_dev.fix_cap, dzfx_off_at(m));
  s.t_h2d += now_s() - t0;
  t0 = now_s();
  uint32_t count = 0;
  const dzfx_arrays starts = {(uint32_t *)g_dev.fix, NULL, NULL};
  int rc = fixup_build_dev(&v, &s, bound, starts, 0, &count);
  if (rc == DCTZHIP_E_ARG) return -1;                        /* the streams disagree with each other */
  if (rc != DCTZHIP_OK) die("dctzhip_fixup_build");
  const size_t payload = dzfx_payload_bytes(m, count, ts);
  if (count) {
    grow(&g_dev.fix, &g_dev.fix_cap, payload);
    rc = fixup_build_dev(&v, &s, bound, dzfx_arrays_at(g_dev.fix, m, count), count, &count);
    if (rc != DCTZHIP_OK) die("dctzhip_fixup_build");
  }
  const double t1s = now_s();
  const size_t hb = dzfx_header_bytes(nd ? DZFX_VERSION_ND : DZFX_VERSION);
  unsigned char *b = (unsigned char *)calloc(1, hb + payload);
  if (!b) { fprintf(stderr, "Out of memory: correction list\n"); exit(1); }
  if (nd) dzfx_write_header_nd(b, v.is_d, nd, v.dims, n_ref, nblk, count, bound);
  else dzfx_write_header(b, v.is_d, n, count, bound);
  /* the three arrays sit on the device as they sit in the blob; the padding between them is cleared afterwards */
  if (dctzhip_memcpy_d2h(c, b + hb, g_dev.fix, payload) != DCTZHIP_OK) die("D2H correction list");
  memset(b + hb + (m + 1) * sizeof(uint32_t), 0, dzfx_off_at(m) - (m + 1) * sizeof(uint32_t));
  memset(b + hb + dzfx_off_at(m) + (size_t)count * sizeof(uint16_t), 0, dzfx_val_at(m, count) - dzfx_off_at(m) - (size_t)count * sizeof(uint16_t));
  *blob = b; *blob_bytes = hb + payload;
  part_times(&s, t_begin, t0, t1s);
  return 1;
}

/* ------------------------------------------ dctz_compress_masked, dctz_decompress_masked -- */
/* The array goes to the device, dctzhip_mask_build fills it in place and makes the mask, both come back, and the container
 * is then simply dctz_compress of the filled array -- byte for byte that call's output, the in-place x /= sf of the caller's
 * buffer included (as dctz_compress_psnr: the second H2D copy inside dctz_compress is the price of that identity).  The mask
 * words leave as one zlib stream behind the blob's header (csrc/dctz_mask_blob.h). */
static int masked_args_ok(const t_var *var, const t_var *var_z, const size_t *outSize, const dctz_missing *miss, void **mask_blob,
                          const size_t *mask_bytes) {
  if (!var || !var_z || !outSize || !miss || !mask_blob || !mask_bytes) return 0;
  if (var->datatype != DOUBLE && var->datatype != FLOAT) return 0;
  if (!var_bytes((t_var *)var)) return 0;
  if (miss->flags == 0 || (miss->flags & ~DZMK_FLAGS_ALL)) return 0;
  if ((miss->flags & DCTZHIP_MISS_VALUE) && isnan(miss->value)) return 0;
  if ((miss->flags & DCTZHIP_MISS_ABS_GE) && !(miss->limit > 0.0 && !isinf(miss->limit))) return 0;
  return 1;
}

/* The checked call: nd = 0 fills inside flat blocks, nd = 2 / 3 inside the tiles of the array dims, which dctz_compress is
 * then asked to compress in tiles. */
static int compress_masked_checked(t_var *var, int nd, const size_t *dims, int N, size_t *outSize, t_var *var_z, double error_bound,
                                   const dctz_missing *miss, double fill, void **mask_blob, size_t *mask_bytes) {
  const int is_d = (var->datatype == DOUBLE), dtype = is_d ? DCTZHIP_F64 : DCTZHIP_F32;
  void *host = var_bytes(var);
  const size_t n = (size_t)N, ts = is_d ? sizeof(double) : sizeof(float), words = dctzhip_mask_words(n);
  dctzhip_ctx *c = ctx();
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.fix, &g_dev.fix_cap, words * sizeof(uint64_t));
  if (dctzhip_memcpy_h2d(c, g_dev.in, host, n * ts) != DCTZHIP_OK) die("H2D");
  dctzhip_missing m;
  m.flags = miss->flags; m.value = miss->value; m.limit = miss->limit;
  uint64_t count = 0;
  if (nd) {
    if (dctzhip_mask_build_nd(c, g_dev.in, nd, dims, dtype, &m, (uint64_t *)g_dev.fix, g_dev.in, &count) != DCTZHIP_OK) die("dctzhip_mask_build_nd");
  } else if (dctzhip_mask_build(c, g_dev.in, n, dtype, &m, (uint64_t *)g_dev.fix, g_dev.in, &count) != DCTZHIP_OK) {
    die("dctzhip_mask_build");
  }
  uint64_t *w = (uint64_t *)malloc(words * sizeof(uint64_t));
  uLongf zbytes = compressBound((uLong)(words * sizeof(uint64_t)));
  unsigned char *b = (unsigned char *)malloc(DZMK_HEADER_BYTES + (size_t)zbytes);
  if (!w || !b) { fprintf(stderr, "Out of memory: mask\n"); exit(1); }
  if (dctzhip_memcpy_d2h(c, host, g_dev.in, n * ts) != DCTZHIP_OK) die("D2H filled array");
  if (dctzhip_memcpy_d2h(c, w, g_dev.fix, words * sizeof(uint64_t)) != DCTZHIP_OK) die("D2H mask");
  if (compress2(b + DZMK_HEADER_BYTES, &zbytes, (const Bytef *)w, (uLong)(words * sizeof(uint64_t)), DZMK_ZLIB_LEVEL) != Z_OK) die("compress2 (mask)");
  free(w);
  dzmk_write_header(b, is_d, miss->flags, n, (size_t)count, fill, (size_t)zbytes);
  if (nd && dctz_set_block_dims(nd, dims) != 0) { free(b); return -1; }
  const int ret = dctz_compress(var, N, outSize, var_z, error_bound);
  if (ret != 1) { free(b); return ret; }
  *mask_blob = b; *mask_bytes = DZMK_HEADER_BYTES + (size_t)zbytes;
  return 1;
}

int dctz_compress_masked(t_var *var, int N, size_t *outSize, t_var *var_z, double error_bound, const dctz_missing *miss, double fill,
                         void **mask_blob, size_t *mask_bytes) {
  if (N <= 0 || !masked_args_ok(var, var_z, outSize, miss, mask_blob, mask_bytes)) return -1;
  if (g_nd || (getenv("DCTZ_BLOCK_DIMS") && *getenv("DCTZ_BLOCK_DIMS"))) return -1;   /* flat blocks only: the fill runs over them */
  return compress_masked_checked(var, 0, NULL, N, outSize, var_z, error_bound, miss, fill, mask_blob, mask_bytes);
}

/* The same for an array compressed in tiles: dctzhip_mask_build_nd fills inside the tiles, and the container is byte for byte
 * dctz_set_block_dims(ndims, dims) + dctz_compress of the filled array.  A request of the caller's that is still pending is
 * not consumed: the call is refused. */
int dctz_compress_masked_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, double error_bound,
                            const dctz_missing *miss, double fill, void **mask_blob, size_t *mask_bytes) {
  if (mask_blob) *mask_blob = NULL;
  if (!masked_args_ok(var, var_z, outSize, miss, mask_blob, mask_bytes)) return -1;
  if ((ndims != 2 && ndims != 3) || !dims || g_nd) return -1;
  size_t n = 1;
  for (int i = 0; i < ndims; i++) {
    if (dims[i] == 0 || dims[i] > 0x7FFFFFFFu || n > (size_t)0x7FFFFFFF / dims[i]) return -1;
    n *= dims[i];
  }
  if (dctzhip_nd_blocks(ndims, dims) == 0) return -1;      /* (more tiles than the streams can number) */
  return compress_masked_checked(var, ndims, dims, (int)n, outSize, var_z, error_bound, miss, fill, mask_blob, mask_bytes);
}

/* The mask words of a checked blob, inflated (malloc'd), or NULL if the payload is not exactly those words */
static unsigned char *mask_words_of(const void *mask_blob, const dzmk_header *mh) {
  const size_t wbytes = (size_t)mh->words * sizeof(uint64_t);
  /* (one byte of room more: a payload that holds more than the words must not pass for one that holds them) */
  unsigned char *w = (unsigned char *)malloc(wbytes + 8);
  if (!w) { fprintf(stderr, "Out of memory: mask\n"); exit(1); }
  uLongf got = (uLongf)(wbytes + 8);
  if (uncompress(w, &got, (const Bytef *)mask_blob + DZMK_HEADER_BYTES, (uLong)mh->payload_bytes) != Z_OK || (size_t)got != wbytes) { free(w); return NULL; }
  return w;
}

/* dctz_decompress, then the correction list if one is given, then the mask.  Both blob headers are held against the
 * container's before anything else happens, and the mask's payload must inflate to exactly its words. */
int dctz_decompress_masked(t_var *var_z, const void *mask_blob, size_t mask_bytes, const void *fix_blob, size_t fix_bytes, t_var *var_r) {
  dzc_view v;
  if (!var_z || !var_bytes(var_z)) return -1;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype);
  dzmk_header mh;
  dzfx_header fh;
  if (v.nd != 0 || v.n == 0 || !var_r) return -1;
  if (dzmk_check(mask_blob, mask_bytes, v.is_d, v.n, &mh) != 0) return -1;
  if (fix_blob && dzfx_check(fix_blob, fix_bytes, v.is_d, v.n, &fh) != 0) return -1;
  unsigned char *w = mask_words_of(mask_blob, &mh);
  if (!w) return -1;
  const int ret = decompress_whole(var_z, var_r, (const unsigned char *)fix_blob, (const uint64_t *)w, mh.fill);
  free(w);
  return ret;
}

/* The same for a DZND container: the mask covers the array's prod dims elements in C order, as the reconstruction lies on the
 * device, and a correction blob is the tiled kind (dctz_decompress_bounded's checks). */
int dctz_decompress_masked_nd(t_var *var_z, const void *mask_blob, size_t mask_bytes, const void *fix_blob, size_t fix_bytes, t_var *var_r) {
  dzc_view v;
  if (!var_z || !var_bytes(var_z)) return -1;
  dzc_header(&v, var_bytes(var_z), DCTZ_QT, (int)var_z->datatype);
  dzmk_header mh;
  dzfx_header_nd nh;
  if (v.nd == 0 || v.n == 0 || !var_r || dzc_geometry(&v) != 0) return -1;
  if (dzmk_check(mask_blob, mask_bytes, v.is_d, v.n, &mh) != 0) return -1;
  if (fix_blob && dzfx_check_nd(fix_blob, fix_bytes, v.is_d, v.nd, v.dims, v.n, v.nblk, &nh) != 0) return -1;   /* (a flat blob: its version) */
  unsigned char *w = mask_words_of(mask_blob, &mh);
  if (!w) return -1;
  const int ret = decompress_whole(var_z, var_r, (const unsigned char *)fix_blob, (const uint64_t *)w, mh.fill);
  free(w);
  return ret;
}

/* ------------------------------------------------------ calc_data_stat ----- */
/* util.c:12-44 on the GPU: max/min by tree reduction (order-independent),
 * the sum by the serial-order kernel so that mean is bit-identical. */
void calc_data_stat(t_var *in, t_bstat *bs, int N) {
  const int is_d = (in->datatype == DOUBLE);
  const size_t ts = is_d ? sizeof(double) : sizeof(float);
  const size_t n = (size_t)N;
  dctzhip_ctx *c = ctx();
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  if (dctzhip_memcpy_h2d(c, g_dev.in, var_bytes(in), n * ts) != DCTZHIP_OK) die("H2D");
  dctzhip_cinfo info;
  double mean = 0.0;
  if (dctzhip_serial_mean_begin(c, g_dev.in, n, is_d ? DCTZHIP_F64 : DCTZHIP_F32) != DCTZHIP_OK) die("serial mean");
  if (dctzhip_stats(c, g_dev.in, n, is_d ? DCTZHIP_F64 : DCTZHIP_F32, &info) != DCTZHIP_OK) die("dctzhip_stats");
  if (dctzhip_serial_mean_end(c, &mean) != DCTZHIP_OK) die("serial mean");
  /* util.c:18-19: max and min start from |x[0]|, and a NaN there stays (dctzhip_stats passes a NaN over wherever it stands) */
  if (is_d ? isnan(in->buf.d[0]) : isnan(in->buf.f[0])) { info.max_abs = info.min_abs = (double)NAN; info.sf = (double)NAN; }
  if (is_d) { bs->max.d = info.max_abs; bs->min.d = info.min_abs; bs->mean.d = mean; bs->sf.d = info.sf; }
  else { bs->max.f = (float)info.max_abs; bs->min.f = (float)info.min_abs; bs->mean.f = (float)mean; bs->sf.f = (float)info.sf; }
}

/* ------------------------------------------------------------- gen_bins ---- */
/* binning.c:12-50: centre of bin b is (+1,-1,+2,-2,...) times the bin width. */
void gen_bins(double min, double max, double *bin_center, int nbins, double error_bound) {
  (void)min; (void)max;
  const double bin_width = error_bound * 2 * BRSF;
  bin_center[0] = 0.0;
  for (int b = 1; b < nbins; b++) {
    const int signed_step = (b & 1) ? (b / 2) + 1 : -(b / 2);
    bin_center[b] = signed_step * bin_width;
  }
}

void gen_bins_f(float min, float max, float *bin_center, int nbins, float error_bound) {
  (void)min; (void)max;
  const float bin_width = error_bound * 2 * BRSF;
  bin_center[0] = 0.0;
  for (int b = 1; b < nbins; b++) {
    const int signed_step = (b & 1) ? (b / 2) + 1 : -(b / 2);
    bin_center[b] = signed_step * bin_width;
  }
}

/* ------------------------------------------------------------- calc_psnr --- */
/* util.c:54-104 (harness metric; not part of the codec). */
/* Arrays of at least this many elements take the GPU reductions (dctzhip_psnr_terms: min, max and max |e| exact,
 * the sum of squares in tree order, 1e-15 relative to the serial loop); DCTZ_PSNR_HOST=1 keeps the loop below. */
#define PSNR_GPU_MIN (1 << 16)
double calc_psnr(t_var *var, t_var *var_r, int N, double error_bound) {
  (void)error_bound;
  double lo, hi, worst = 0.0, sq = 0.0;
  if (N >= PSNR_GPU_MIN && !getenv("DCTZ_PSNR_HOST")) {
    const int is_d = var->datatype == DOUBLE;
    const size_t bytes = (size_t)N * (is_d ? sizeof(double) : sizeof(float));
    dctzhip_ctx *c = ctx();
    double t[4];
    grow(&g_dev.in, &g_dev.in_cap, bytes);
    grow(&g_dev.out, &g_dev.out_cap, bytes);
    if (dctzhip_memcpy_h2d(c, g_dev.in, var_bytes(var), bytes) != DCTZHIP_OK || dctzhip_memcpy_h2d(c, g_dev.out, var_bytes(var_r), bytes) != DCTZHIP_OK)
      die("H2D");
    if (dctzhip_psnr_terms(c, g_dev.in, g_dev.out, (size_t)N, is_d ? DCTZHIP_F64 : DCTZHIP_F32, t) != DCTZHIP_OK)
      die("dctzhip_psnr_terms");
    lo = t[0]; hi = t[1]; worst = t[2]; sq = t[3];
  } else if (var->datatype == DOUBLE) {
    const double *x = var->buf.d, *r = var_r->buf.d;
    lo = hi = x[0];
    for (int i = 1; i < N; i++) { if (x[i] > hi) hi = x[i]; if (x[i] < lo) lo = x[i]; }
    for (int i = 0; i < N; i++) {
      const double e = x[i] - r[i];
      if (fabs(e) > worst) worst = fabs(e);
      sq += e * e;
    }
  } else {
    const float *x = var->buf.f, *r = var_r->buf.f;
    lo = hi = x[0];
    for (int i = 1; i < N; i++) { if (x[i] > hi) hi = x[i]; if (x[i] < lo) lo = x[i]; }
    for (int i = 0; i < N; i++) {
      const float e = x[i] - r[i];
      if (fabs(e) > worst) worst = fabs(e);
      sq += (e * e);
    }
  }
  const double rmse = sqrt(sq / N), range = hi - lo;
  printf("Max relative error = %.6f\n", worst / range); /* util.c:95 */
  return 20 * log10(range / rmse);
}

/* ------------------------------------------------- dct.h transform layer --- */
/* dct_init / dct_finish keep no state here (the GPU context owns the tables,
 * rebuilt per length on demand); they exist so dct-test.c links and runs. */
void dct_init(int dn) { (void)dn; (void)ctx(); }
void dct_init_f(int dn) { (void)dn; (void)ctx(); }
void dct_finish(void) {}
void dct_finish_f(void) {}
void idct_finish(void) {}
void idct_finish_f(void) {}

static void blocks(void *a, void *b, size_t n, int is_d, int inverse) {
  const size_t ts = is_d ? sizeof(double) : sizeof(float);
  dctzhip_ctx *c = ctx();
  grow(&g_dev.in, &g_dev.in_cap, n * ts);
  grow(&g_dev.out, &g_dev.out_cap, n * ts);
  if (dctzhip_memcpy_h2d(c, g_dev.in, a, n * ts) != DCTZHIP_OK) die("H2D");
  if (dctzhip_dct_blocks(c, g_dev.in, g_dev.out, n, is_d ? DCTZHIP_F64 : DCTZHIP_F32, inverse) != DCTZHIP_OK)
    die("dctzhip_dct_blocks");
  if (dctzhip_memcpy_d2h(c, b, g_dev.out, n * ts) != DCTZHIP_OK) die("D2H");
}

void dctz_dct_blocks(double *a, double *b, size_t n, int inverse) { blocks(a, b, n, 1, inverse); }
void dctz_dct_blocks_f(float *a, float *b, size_t n, int inverse) { blocks(a, b, n, 0, inverse); }

/* one block of length dn per call, like the reference (dct.c:55, :115).  The reference transforms ANY length with one
 * length-dn plan; the codec only ever uses dn <= BLK_SZ = 64 (dctz.h:28), which is what the GPU tables cover: a longer
 * block is refused loudly instead of being cut into 64-element blocks (a different transform). */
/* ... on the HOST (dct_host.cpp): the caller's block is in host memory and is read back at once; the product's own lane
 * flow (dct64_block.h, the code one GPU lane runs) compiled for the CPU gives bit for bit what dctz_dct_blocks() returns
 * from the device, without an H2D copy, a launch and a D2H copy per 512 bytes.  (DCTZ_BLOCK_ON_GPU=1: through the GPU.) */
void dctz_host_block_f64(const double *a, double *b, int dn, int inverse);
void dctz_host_block_f32(const float *a, float *b, int dn, int inverse);
static void one_block(void *a, void *b, int dn, int is_d, int inverse) {
  static int on_gpu = -1;
  if (dn < 1 || dn > BLK_SZ) {
    fprintf(stderr, "libdctz: %s with dn = %d: only block lengths 1..%d are supported\n", inverse ? "ifft_idct" : "dct_fftw", dn, BLK_SZ);
    exit(1);
  }
  if (on_gpu < 0) { const char *e = getenv("DCTZ_BLOCK_ON_GPU"); on_gpu = e && atoi(e) ? 1 : 0; }
  if (on_gpu) { blocks(a, b, (size_t)dn, is_d, inverse); return; }
  if (is_d) dctz_host_block_f64((const double *)a, (double *)b, dn, inverse);
  else dctz_host_block_f32((const float *)a, (float *)b, dn, inverse);
}
void dct_fftw(double *a, double *b, int dn, int nblk) { (void)nblk; one_block(a, b, dn, 1, 0); }
void dct_fftw_f(float *a, float *b, int dn, int nblk) { (void)nblk; one_block(a, b, dn, 0, 0); }
void ifft_idct(int dn, double *a, double *data) { one_block(a, data, dn, 1, 1); }
void ifft_idct_f(int dn, float *a, float *data) { one_block(a, data, dn, 0, 1); }
