/*
 * dctz.h -- public API of the drop-in host library libdctz-{ec,qt}.so.
 *
 * Binary- and source-compatible with the reference's dctz.h (types, constants
 * and prototypes at dctz.h:28-128) and dct.h (dct.h:17-27), so a caller such as
 * dctz-test.c or the Z-checker glue compiles and links against this library
 * unchanged.  The block-DCT + binning stages behind dctz_compress() /
 * dctz_decompress() run on an MI355X through include/dctz_hip.h; the zlib tail
 * and the container stay on the host.
 *
 * Build-time variants, as in the reference Makefile:12-17: USE_TRUNCATE is
 * always defined (DC / AC_exact stored as float); USE_QTABLE selects the QT
 * library and adds header.bindex_count.
 *
 * Differences from the reference header: fftw3.h is not included (nothing here
 * needs FFTW), and the never-defined ceili() prototype (dctz.h:122) is omitted.
 */
#ifndef _DCTZ_H_
#define _DCTZ_H_

#include <math.h>
#include <memory.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "zlib.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCTZ_VERSION "0.2.2"          /* wire-format version we interoperate with */
#define DCTZ_VERSION_MAJOR 0
#define DCTZ_VERSION_MINOR 2
#define DCTZ_VERSION_PATCH 2

#ifndef M_PI
#define M_PI 3.14159265358979323846   /* dct.h:13-15 */
#endif

#define BLK_SZ 64                     /* elements per block              (dctz.h:28) */
#define BRSF 1.0                      /* bin range scaling factor        (dctz.h:29) */
#define SF_ADJ_AMT 1                  /* scaling factor exponent offset  (dctz.h:30) */

#ifndef MAX
#define MAX(a, b) ({ __typeof__(a) a_ = (a); __typeof__(b) b_ = (b); a_ > b_ ? a_ : b_; })
#endif
#ifndef MIN
#define MIN(a, b) ({ __typeof__(a) a_ = (a); __typeof__(b) b_ = (b); a_ < b_ ? a_ : b_; })
#endif
#define CEIL(a, b) (a + b - 1) / b    /* as in dctz.h:42 (unparenthesised) */

/* element type tag (dctz.h:44-47) */
typedef enum { FLOAT = 0, DOUBLE } t_datatype;

/* a typed view of a caller-owned buffer (dctz.h:49-59); 32 bytes on LP64 */
typedef struct {
  t_datatype datatype;
  double err_bound;
  char *var_name;
  union {
    float *f;
    double *d;
  } buf;
} t_var;

typedef unsigned char t_bin_id;                 /* dctz.h:63 */
#define NBITS (sizeof(t_bin_id) << 3)           /* dctz.h:65 */
#define NBINS ((1 << (NBITS)) - 1)              /* 255; id 255 = "stored exactly" */

/* statistics of one array (dctz.h:68-94) */
typedef struct {
  union { double d; float f; } mean;
  union { double d; float f; } min;
  union { double d; float f; } max;
  union { double d; float f; } range;
  union { double d; float f; } sf;
} t_bstat;

/* container header, 56 bytes, native endianness (dctz.h:96-119) */
struct header {
  t_datatype datatype;
  unsigned int num_elements;
  double error_bound;
  unsigned int tot_AC_exact_count;
  union { double d; float f; } scaling_factor;
  union { double d; float f; } mean;
  unsigned int bindex_sz_compressed;
  unsigned int DC_sz_compressed;
  unsigned int AC_exact_sz_compressed;
#ifdef USE_QTABLE
  unsigned int bindex_count;
#endif
};

/* dctz.h:121-128 */
void calc_data_stat(t_var *in, t_bstat *bs, int N);
void gen_bins(double min, double max, double *bin_center, int nbins, double error_bound);
void gen_bins_f(float min, float max, float *bin_center, int nbins, float error_bound);
void *compress_thread(void *arg);
int dctz_compress(t_var *var, int N, size_t *outSize, t_var *var_z, double error_bound);
int dctz_decompress(t_var *var_z, t_var *var_r);
double calc_psnr(t_var *var, t_var *var_r, int N, double error_bound);

/* dct.h:17-27 -- per-block transform entry points (driven by dct-test.c) */
void dct_init(int dn);
void dct_init_f(int dn);
void dct_fftw(double *a, double *b, int dn, int nblk);
void dct_fftw_f(float *a, float *b, int dn, int nblk);
void ifft_idct(int dn, double *a, double *data);
void ifft_idct_f(int dn, float *a, float *data);
void dct_finish(void);
void dct_finish_f(void);
void idct_finish(void);
void idct_finish_f(void);

/* ---- additions (not in the reference) ------------------------------------ */
/* Whole-array forms of dct_fftw / ifft_idct: every 64-element block of a[0..n)
 * (last one of length n % 64) in one GPU pass; what dct-test.c:81-89 / 144-152
 * compute with a loop. */
void dctz_dct_blocks(double *a, double *b, size_t n, int inverse);
void dctz_dct_blocks_f(float *a, float *b, size_t n, int inverse);
/* Lists of arrays (ADDITIONS, round 4).  The reference's own workloads are lists of small arrays, one dctz_compress()
 * call -- one process -- per array (tests/test-dctz.sh:13-56 over tests/list-msst19.txt:1-6).  These take k arrays at once:
 * one copy in, ONE batch launch (every array with its own calc_data_stat, scaling factor, bin ranges, tot_AC_exact_count
 * and QT table: dctz-comp-lib.c:186 onwards couples nothing across arrays), one copy back, and the reference's tail -- one
 * single-shot deflate per section, dctz-comp-lib.c:620-732 -- for all 3 k sections on a pool of host threads.  Arguments
 * as dctz_compress()'s, per array: vars[i] (N[i] elements, scaled in place by its sf on return), vars_z[i] (>= N[i] *
 * type_size bytes), outSizes[i], error_bounds[i].  Container i is byte for byte what dctz_compress(vars[i], ...) writes
 * with the default tail.  Flat blocks only.  dctz_decompress_batch() is the mirror image (any flat containers).
 * Arrays may share bytes (one t_var twice, two t_vars over one buffer): the result -- containers, outSizes and the final
 * contents of every array -- is then that of the loop of dctz_compress(vars[i], ...) in index order, where a later call
 * reads what an earlier one's in-place scaling left; such a list is run as that loop. */
int dctz_compress_batch(int k, t_var *const *vars, const int *N, size_t *outSizes, t_var *const *vars_z, const double *error_bounds);
int dctz_decompress_batch(int k, t_var *const *vars_z, t_var *const *vars_r);
/* Compression to a target PSNR (ADDITION, EC).  The error bound is chosen on the device -- rate-distortion probe, then
 * compress, decode and measure, stepping down a fixed grid of bounds on a miss (include/dctz_hip.h: dctzhip_compress_psnr) --
 * and the container is then dctz_compress(var, N, outSize, var_z, *error_bound_used): byte for byte that call's output,
 * the in-place x /= sf of var->buf included.  Its calc_psnr against the original is >= target_psnr.  Returns what
 * dctz_compress returns (1), or without writing anything: DCTZHIP_E_BOUND (-2) when no bound >= 1e-6 reaches the
 * target, DCTZHIP_E_ARG (-1) for bad arguments, a constant array or a NaN (PSNR undefined), pending multi-dimensional
 * blocks (flat blocks only), and always in the QT library (its bin widths come from a whole-array table). */
int dctz_compress_psnr(t_var *var, int N, size_t *outSize, t_var *var_z, double target_psnr, double *error_bound_used);
/* Its twin for an array compressed in 8 x 8 (ndims = 2) or 4 x 4 x 4 (ndims = 3) tiles (ADDITION, EC).  The bound is chosen by
 * dctzhip_compress_psnr_nd (the same grid and search over the array's own prod dims elements, no edge padding), and the
 * container is then dctz_set_block_dims(ndims, dims) + dctz_compress(var, prod dims, outSize, var_z, *error_bound_used):
 * byte for byte those calls' output, the in-place x /= sf of var->buf included.  Returns what dctz_compress returns (1), or
 * without writing anything: DCTZHIP_E_BOUND (-2) when no bound >= 1e-6 reaches the target, DCTZHIP_E_ARG (-1) for bad
 * arguments, ndims other than 2 or 3, an extent of 0, a product or tile count beyond an int, a constant array or a NaN, while
 * a dctz_set_block_dims request of the caller's is pending (it stays pending), and always in the QT library.  Every refusal
 * that does not need the data comes before a device is asked for. */
int dctz_compress_psnr_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, double target_psnr,
                          double *error_bound_used);
/* Part of a container (ADDITION, EC and QT builds): elements [lo, hi), 0 <= lo < hi <= N, of what dctz_decompress(var_z,
 * ...) reconstructs, bit for bit, into var_r->buf (allocated by the caller: at least hi - lo elements of the container's
 * type).  Returns 1 like dctz_decompress, or -1 for a bad range, a multi-dimensional (DZND) container -- its element
 * order is not the block order --, and a container whose sections do not inflate as far as the range needs or whose bin
 * ids disagree with tot_AC_exact_count.  It inflates no more than the range needs: bin_index up to min(N, 4096 t1)
 * (t1 = ceil(hi / 4096): the flags in front give the range's place in AC_exact), DC up to the range's last block,
 * AC_exact up to the exception index's idx[t1] (include/dctz_hip.h: dctzhip_ac_index, built on the device from that
 * bin_index prefix).  Plain zlib sections go through a streaming inflate that stops there; in a container with the DZIX
 * chunk index the chunks that lie wholly beyond it are not inflated at all.  Nothing of the container is validated
 * beyond that. */
int dctz_decompress_range(t_var *var_z, size_t lo, size_t hi, t_var *var_r);
/* A box of a container (ADDITION, EC and QT builds): the array as an ndim-dimensional array in C order (1 <= ndim <= 4,
 * prod dims = N, last dimension fastest), elements lo[i] <= c[i] < hi[i], dense and in C order into var_r->buf (allocated
 * by the caller: prod (hi[i] - lo[i]) elements).  Each is bit for bit the element dctz_decompress reconstructs at those
 * coordinates.  Returns 1, or -1 for a bad box (ndim, a null pointer, lo[i] >= hi[i], hi[i] > dims[i]), prod dims != N, a
 * DZND container and streams that disagree with each other -- dctz_decompress_range's return values.  It inflates what
 * dctz_decompress_range(first box element, last box element + 1) inflates and no more; on the device only the tiles that
 * hold box elements are decoded, once each (include/dctz_hip.h: dctzhip_decompress_box), and only the box is copied back. */
int dctz_decompress_box(t_var *var_z, int ndim, const size_t *dims, const size_t *lo, const size_t *hi, t_var *var_r);
/* k boxes of ONE container in one call (ADDITION, EC and QT builds), 1 <= k <= 4096: lo and hi hold k rows of ndim entries,
 * var_r[j]->buf (allocated by the caller) receives box j, the bytes dctz_decompress_box gives for it.  Boxes may overlap or
 * repeat.  The container is gone through ONCE: the sections are inflated up to what the last element of any box needs (plain
 * and DZIX, as dctz_decompress_range(smallest first box element, largest last box element + 1) would), one exception index
 * is built, one device call (include/dctz_hip.h: dctzhip_decompress_boxes) decodes the hit tiles of every box into one
 * device arena, and k copies bring the boxes back.  Return values and refusals are dctz_decompress_box's, for any box of
 * the list (nothing is written then); a k outside 1 .. 4096 and a null lo, hi, var_r or var_r[j] return -1 as well. */
int dctz_decompress_boxes(t_var *var_z, int ndim, const size_t *dims, int k,
                          const size_t *lo, const size_t *hi,   /* k rows of ndim entries */
                          t_var *const *var_r);                 /* k caller-allocated outputs */
/* A box of a container compressed in tiles (ADDITION, EC and QT builds): var_z is a DZND container (dctz_set_block_dims +
 * dctz_compress); its geometry and extents come from the container.  Elements lo[i] <= c[i] < hi[i] (2 or 3 entries, as the
 * container has dimensions), dense and in C order into var_r->buf (allocated by the caller); each is bit for bit the element
 * dctz_decompress reconstructs at those coordinates.  Returns 1, or -1 for a flat container, a bad box (a null pointer,
 * lo[i] >= hi[i], hi[i] > dims[i]) and streams that disagree with each other -- dctz_decompress_box's conventions.  The
 * blocks that intersect the box are a box of the row-major block grid; the call inflates what the stream positions [64 *
 * first such block, 64 * (last + 1)) need, exactly as dctz_decompress_range would for a flat container, and no more; on the
 * device only the stream tiles (64 blocks) that hold such a block are decoded, once each (include/dctz_hip.h:
 * dctzhip_decompress_box_nd), and only the box is copied back.  dctz_decompress_range and dctz_decompress_box keep
 * refusing DZND containers. */
int dctz_decompress_box_nd(t_var *var_z, const size_t *lo, const size_t *hi, t_var *var_r);
/* k boxes of ONE container compressed in tiles in one call (ADDITION, EC and QT builds), 1 <= k <= 4096: lo and hi hold k
 * rows of as many entries as the container has dimensions, var_r[j]->buf (allocated by the caller) receives box j, the
 * bytes dctz_decompress_box_nd gives for it.  Boxes may overlap or repeat.  The container is gone through ONCE: the
 * sections are inflated up to what the stream positions [64 * first intersecting block of any box, 64 * (last intersecting
 * block of any box + 1)) need (plain and DZIX), one exception index is built, one device call (include/dctz_hip.h:
 * dctzhip_decompress_boxes_nd) decodes the hit stream tiles of every box into one device arena, and k copies bring the
 * boxes back.  Return values are dctz_decompress_box_nd's, for any box of the list (nothing is written then); a flat
 * container, a k outside 1 .. 4096 and a null lo, hi, var_r or var_r[j] return -1 as well.  dctz_decompress_boxes keeps
 * refusing DZND containers. */
int dctz_decompress_boxes_nd(t_var *var_z, int k,
                             const size_t *lo, const size_t *hi,   /* k rows of the container's dimensions */
                             t_var *const *var_r);                 /* k caller-allocated outputs */
/* The whole array at reduced resolution (ADDITION, EC and QT builds): an overview at 1 / factor of the resolution along
 * every axis, computed from the low coefficients of every block without decoding the array (include/dctz_hip.h:
 * dctzhip_decompress_coarse / dctzhip_decompress_coarse_nd hold the definition).  var_z is a flat container (factor 2, 4,
 * 8, 16, 32 or 64; var_r->buf receives ceil(n / factor) elements) or a DZND container (2-D: factor 2, 4 or 8; 3-D: 2 or 4;
 * var_r->buf receives a dense C-order array of extents ceil(dims[i] / factor)); var_r->buf is allocated by the caller.  With
 * factor equal to the block edge (64; 8 | 4) -- and, for a flat container, n a multiple of 64 -- only the DC section is
 * inflated; otherwise the three sections are, and the exception index is built once.  Only the coarse array is copied back.
 * Returns 1, or -1 for a bad factor, a null var_r and streams that disagree with each other -- dctz_decompress_box's
 * conventions. */
int dctz_decompress_coarse(t_var *var_z, int factor, t_var *var_r);
/* A box of that, for DZND containers (ADDITION, EC and QT builds): a window at zoom level `factor` (include/dctz_hip.h:
 * dctzhip_decompress_coarse_box_nd).  lo / hi are in COARSE coordinates, lo[i] < hi[i] <= ceil(dims[i] / factor), rows of
 * the container's dimensions; var_r->buf, allocated by the caller, receives prod (hi[i] - lo[i]) elements, dense, in C order:
 * byte for byte the slice of what dctz_decompress_coarse returns for the same container and factor.  Only the prefix of the
 * sections the box needs is inflated and uploaded -- bin_index up to the end of the last stream tile that may hold a cell of
 * the box, DC up to the last block of the box; with factor equal to the block edge that DC prefix alone -- the exception
 * index is built once, and only the box is copied back.  Returns 1, or -1 for a flat container, a bad factor, a null lo, hi
 * or var_r, a box that is not inside the coarse extents and streams that disagree with each other. */
int dctz_decompress_coarse_box_nd(t_var *var_z, int factor, const size_t *lo, const size_t *hi, t_var *var_r);
/* k such boxes of ONE DZND container at ONE factor in one call (ADDITION, EC and QT builds), 1 <= k <= 4096: lo and hi hold k
 * rows of as many entries as the container has dimensions, in COARSE coordinates; var_r[j]->buf (allocated by the caller)
 * receives box j, the bytes dctz_decompress_coarse_box_nd gives for it.  Boxes may overlap or repeat.  The container is gone
 * through ONCE: bin_index is inflated up to the end of the last candidate stream tile of any box and DC up to the last block
 * of any box (plain and DZIX) -- with factor equal to the block edge that DC prefix alone --, one exception index is built,
 * one device call (include/dctz_hip.h: dctzhip_decompress_coarse_boxes_nd) decodes the hit stream tiles of every box into one
 * device arena, and k copies bring the boxes back.  Return values are dctz_decompress_coarse_box_nd's, for any box of the list
 * (nothing is written then); a k outside 1 .. 4096 and a null lo, hi, var_r or var_r[j] return -1 as well. */
int dctz_decompress_coarse_boxes_nd(t_var *var_z, int factor, int k, const size_t *lo, const size_t *hi, t_var *const *var_r);
/* Verify and survey without a reconstruction (ADDITION, EC and QT builds; include/dctz_hip.h: dctzhip_tile_summary holds the
 * definition).  One record per 4096 elements of what dctz_decompress would rebuild from var_z -- its minimum, maximum, sum
 * and sum of squares -- and, with var_ref, the minimum and maximum of the original, max |x - r| and sum (x - r)^2 of the
 * tile: where the compression is worst.  var_ref->buf is the caller's UNSCALED original, N_ref elements (ignored when
 * var_ref is NULL): dctz_compress has divided the array it was given by sf in place, so keep a copy (or multiply back)
 * before asking.  tiles (or NULL) receives ceil(n / 4096) records, total (or NULL) the records joined; calc_psnr of the
 * pair is 20 log10((total->xmax - total->xmin) / sqrt(total->esq / n)).  The three sections are inflated, the exception
 * index is built once, the original is uploaded when given; records and total alone are copied back -- no reconstruction
 * buffer exists on either side.  Returns 1, or -1 for a DZND container, a null total with null tiles, a reference of
 * another type or length and streams that disagree with each other -- dctz_decompress_box's conventions. */
typedef struct {             /* include/dctz_hip.h: dctzhip_tile_summary_t */
  double rmin, rmax, rsum, rsq;
  double xmin, xmax, emax, esq;
} dctz_tile_summary_t;
int dctz_tile_summary(t_var *var_z, t_var *var_ref /* or NULL */, int N_ref, dctz_tile_summary_t *tiles /* host, or NULL */,
                      dctz_tile_summary_t *total);
/* dctz_tile_summary for a DZND container (ADDITION, EC and QT builds; include/dctz_hip.h: dctzhip_tile_summary_nd holds the
 * definition and the order of the sums).  Geometry and extents come from the container; the records are per stream tile (64
 * blocks of 8 x 8 / 4 x 4 x 4, row-major over the block grid) over the array's own elements -- the edge padding of the
 * streams enters nothing.  var_ref->buf is the UNSCALED original in C order, N_ref = prod dims.  tiles (or NULL) receives
 * ceil(64 nblk / 4096) records.  It goes through the same loader as the other partial readers; records and total alone are
 * copied back.  Returns 1, or -1 for a flat container, a null total with null tiles, a reference of another type or length
 * and streams that disagree with each other.  dctz_tile_summary keeps refusing DZND containers. */
int dctz_tile_summary_nd(t_var *var_z, t_var *var_ref /* or NULL */, int N_ref, dctz_tile_summary_t *tiles /* host, or NULL */,
                         dctz_tile_summary_t *total);
/* Point-wise error bound (ADDITION, EC and QT builds, flat and DZND containers; include/dctz_hip.h, "point-wise error bound", holds the
 * definition).  dctz_fixup_build lists every element that dctz_decompress would rebuild from var_z further than `bound`
 * (absolute, in the data's units, >= 0) from the original, with the original's value, in one malloc'd self-describing block
 * that the caller keeps beside the container and frees: "DZFX", version, dtype, n, tiles, count, bound, then fix_start,
 * fix_off padded to 8 bytes, fix_val (csrc/dctz_fixup_blob.h).  var_ref->buf is the caller's UNSCALED original, N_ref elements,
 * as for dctz_tile_summary.  dctz_decompress_bounded is dctz_decompress with that list applied: every element of var_r->buf
 * then has the original's bits or lies within the bound of it.  The .z container does not change and dctz_decompress reads
 * it as before.  The container decides the kind of list, as for dctz_decompress_coarse: for a DZND container (blocks of 8 x 8
 * / 4 x 4 x 4 tiles) var_ref->buf is the array in C order, N_ref the product of its extents, the list runs over the stream
 * positions (the edge padding is never listed) and the blob is version 2 -- the version-1 header with ndims in its zero
 * field, n = the product of the extents and tiles over the 64 nblk stream positions, then the three extents as 64-bit words
 * (unused ones 0), 72 bytes in all; a flat blob stays version 1, byte for byte.  Both return 1, or -1 for a reference of
 * another type or length, a bound that is negative or not finite, a blob whose header does not fit the container (magic,
 * version -- a flat blob with a DZND container and a tiled blob with a flat one --, dtype, ndims, extents, n, sizes, a
 * count above the array's elements -- checked before anything else is done), a list that contradicts itself or the array
 * and streams that disagree with each other. */
int dctz_fixup_build(t_var *var_z, t_var *var_ref, int N_ref, double bound, void **blob, size_t *blob_bytes);
int dctz_decompress_bounded(t_var *var_z, const void *blob, size_t blob_bytes, t_var *var_r);
/* Missing values (ADDITION, EC and QT builds, flat blocks; include/dctz_hip.h, "missing values", holds the definition: the
 * tests, the fill rule, the mask).  dctz_compress_masked marks the elements of var->buf that `miss` selects, fills them with
 * copies of their valid neighbours inside each 64-element block, and compresses the filled array: the container is byte for
 * byte dctz_compress() of that array, and var->buf is left as that call leaves it (filled and divided by sf).  The mask comes
 * back as one malloc'd self-describing block that the caller keeps beside the container and frees: "DZMK", version, dtype,
 * flags, n, count, fill, words, payload bytes (48 bytes), then the mask words as one zlib stream (csrc/dctz_mask_blob.h).
 * dctz_decompress_masked is dctz_decompress, then the correction list of fix_blob if one is given (dctz_fixup_build against
 * the FILLED array), then `fill` written into every missing element.  Both return 1, or -1 for a DZND container or a pending
 * dctz_set_block_dims, a rule that selects no test or an unknown one, a NaN value, a limit that is not finite and > 0, a blob
 * whose header does not fit the container (magic, version, dtype, n, counts, length -- checked before anything else is done)
 * and a payload that does not inflate to exactly the mask's words. */
typedef struct { unsigned flags; double value; double limit; } dctz_missing;   /* flags: DCTZHIP_MISS_* of dctz_hip.h (1 NaN, 2 Inf, 4 == value, 8 |x| >= limit) */
int dctz_compress_masked(t_var *var, int N, size_t *outSize, t_var *var_z, double error_bound, const dctz_missing *miss,
                         double fill, void **mask_blob, size_t *mask_bytes);
int dctz_decompress_masked(t_var *var_z, const void *mask_blob, size_t mask_bytes,
                           const void *fix_blob /* or NULL */, size_t fix_bytes, t_var *var_r);
/* Missing values of an array compressed in tiles (ADDITION, EC and QT builds; include/dctz_hip.h, "missing values of an array
 * compressed in 8 x 8 / 4 x 4 x 4 tiles").  The two calls above keep refusing tiled input; these are their twins.
 * dctz_compress_masked_nd treats var->buf as a row-major array of ndims = 2 or 3 extents, fills the missing elements inside
 * each tile, and compresses the filled array in tiles: the container is byte for byte dctz_set_block_dims(ndims, dims) +
 * dctz_compress() of that array, var->buf is left as that call leaves it, and the blob is the one above with n = prod dims,
 * the mask over the array in C order.  dctz_decompress_masked_nd is dctz_decompress of a DZND container, then the correction
 * list of fix_blob if one is given (the tiled kind: dctz_fixup_build of that container against the FILLED array), then `fill`
 * written into every missing element.  Both return 1, or -1: compress for the argument errors of dctz_compress_masked, for
 * ndims other than 2 or 3, an extent of 0, a product or a tile count beyond an int, and while a dctz_set_block_dims request of
 * the caller's is pending (it stays pending) -- all before a device is asked for, *mask_blob left NULL; decompress for a flat
 * container, a mask blob whose n is not the product of the container's extents, a correction blob that is flat or has other
 * extents (all checked before anything else is done), and a payload that does not inflate to exactly the mask's words. */
int dctz_compress_masked_nd(t_var *var, int ndims, const size_t *dims, size_t *outSize, t_var *var_z, double error_bound,
                            const dctz_missing *miss, double fill, void **mask_blob, size_t *mask_bytes);
int dctz_decompress_masked_nd(t_var *var_z, const void *mask_blob, size_t mask_bytes,
                              const void *fix_blob /* or NULL */, size_t fix_bytes, t_var *var_r);
/* Multi-dimensional blocks (optional; SURVEY section 8 f4 -- NOT in the reference, whose library flattens every
 * array, dctz-test.c:77-91; the hint is its FFTW r2r experiment dct-fftw-test.c:74-97).  The NEXT dctz_compress call
 * treats var->buf as a row-major ndims-dimensional array (ndims = 2: 8 x 8 tiles, ndims = 3: 4 x 4 x 4 tiles, last
 * extent fastest, product = N) and transforms tiles with the separable orthonormal DCT instead of runs of 64
 * consecutive elements; the call after that is flat again.  Environment DCTZ_BLOCK_DIMS="1800x3600" does the same
 * for every call whose N matches (callers that cannot be changed).  ndims <= 1 cancels.  Returns 0, or -1 for
 * bad arguments.
 * Container of such a call: header.datatype carries the geometry in bits 8..15 (DCTZ_GEOM_OF), the three
 * sections cover nblk * 64 positions (edge tiles are padded), and 16 bytes follow the last section:
 * "DZND" + three 32-bit extents.  The reference's decoder cannot read it; dctz_decompress here reads both. */
int dctz_set_block_dims(int ndims, const size_t *dims);
#define DCTZ_GEOM_SHIFT 8
#define DCTZ_GEOM_OF(datatype) (((unsigned)(datatype) >> DCTZ_GEOM_SHIFT) & 0xffu)   /* 0: flat; 2, 3: number of axes */
#define DCTZ_TYPE_OF(datatype) ((t_datatype)((unsigned)(datatype) & 0xffu))
#define DCTZ_ND_MAGIC 0x444E5A44u   /* "DZND" little-endian */
/* Chunk index (optional trailer, written when the entropy stage ran on the GPU: DCTZ_ZLIB_GPU=1).  The three sections
 * are then standard zlib streams whose deflate blocks are independent chunks (header bytes 78 5E instead of zlib's
 * 78 9C; include/dctz_hip.h: dctzhip_deflate), and behind everything else of the container follow
 *   "DZIX" | u32 chunk bytes | u32 chunks of section 0, 1, 2 | u16 compressed bytes of every chunk ... | pad to 4.
 * The reference's reader never looks there (it inflates each section as one stream, dctz-decomp-lib.c:244-322);
 * dctz_decompress here looks for the trailer only when all three sections start 78 5E (zlib itself writes 78 9C at the
 * reference's settings), validates it against the header (chunk counts, sizes that tile each stream exactly up to its
 * 03 00 + adler32) and then inflates the chunks side by side on DCTZ_ZLIB_THREADS host threads (default: the cores) --
 * or on the device with DCTZ_INFLATE_GPU=1; anything inconsistent -- an index that does not describe the sections, a chunk
 * that does not inflate, content whose adler32 is not the stream's -- falls back to the ordinary one-stream inflate, which
 * treats damage as the reference's reader does.
 * dctz_decompress() is not told the size of var_z->buf (dctz.h:127), so it can only TRUST that a container whose three
 * sections start 78 5E is followed by its index (20 bytes + 2 per chunk): for containers of unknown origin -- zlib at levels
 * 2 .. 5 writes 78 5E too -- call dctz_check_container(z, zbytes, ...) first, which has the size and refuses a marked
 * container whose index is missing, cut short or does not tile the sections. */
#define DCTZ_IX_MAGIC 0x58495A44u   /* "DZIX" little-endian */
/* Stage timers of the last dctz_compress / dctz_decompress call, seconds
 * (the reference's -DTIME_DEBUG split, dctz-comp-lib.c:762-773). */
typedef struct {
  double h2d_s, gpu_s, d2h_s, zlib_s, total_s;
} dctz_stage_times;
void dctz_last_stage_times(dctz_stage_times *t);
/* The zlib tail (dctz-comp-lib.c:620-732) as a chunked multi-threaded deflate that still
 * yields ONE standard zlib stream, so dctz-decomp-lib.c:244-322 inflates it unchanged
 * (csrc/pdeflate.c).  dctz_compress uses it when the environment has
 * DCTZ_ZLIB_THREADS > 3; exported for tools that write DCTZ containers themselves.
 * cap >= dctz_pdeflate_bound(n, chunk); returns 0 on success. */
/* Bounds / plausibility check of a DCTZ container held in `zbytes` bytes, to be run before
 * dctz_decompress(), which -- like the reference (dctz-decomp-lib.c:84-100) -- trusts the header.
 * max_elements > 0 additionally bounds N (the size of the caller's output buffer); deep != 0 also
 * inflates the three sections and checks their sizes.  No GPU involved.  The library variant must
 * match the file's (EC vs QT): the QT check expects the trailing table and bindex_count. */
#define DCTZ_CHECK_OK 0
#define DCTZ_CHECK_TRUNCATED (-1)     /* fewer bytes than the header describes                */
#define DCTZ_CHECK_BAD_HEADER (-2)    /* a field is impossible (datatype, N, error bound, cnt) */
#define DCTZ_CHECK_TOO_LARGE (-3)     /* N exceeds max_elements                                */
#define DCTZ_CHECK_BAD_STREAM (-4)    /* a section does not inflate to its expected size       */
int dctz_check_container(const void *z, size_t zbytes, int max_elements, int deep);
size_t dctz_pdeflate_bound(size_t n, size_t chunk);
int dctz_pdeflate(const void *src, size_t n, void *dst, size_t cap, size_t *out_len, int threads, size_t chunk);
void dctz_pdeflate_set_level(int level);   /* 1..9; anything else = zlib's default level (the reference's) */

#ifdef __cplusplus
}
#endif
#endif /* _DCTZ_H_ */
