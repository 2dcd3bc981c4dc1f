/*
 * dctz_container.h -- the layout of a .z container, in one place (internal; format documented in include/dctz.h):
 *
 *   header (56 bytes) | bin_index.z | DC.z | AC_exact.z | [qtable] | ["DZND" + 3 extents] | ["DZIX" chunk index]
 *
 * header, sections, table: the reference's container (dctz.h:96-119, writer dctz-comp-lib.c:775-820, reader
 * dctz-decomp-lib.c:84-100,186-199).  qtable: QT only, 64 entries in the data type.  "DZND": multi-dimensional blocks.
 * "DZIX": sections made by the GPU entropy stage.  Every reader and writer of the drop-in library and the command-line
 * tools goes through this file.  The variant (EC / QT) is an argument, not an #ifdef: the two headers have the same
 * size -- QT's bindex_count sits in what is padding in EC -- and dctz-dump reads both with one binary.
 */
#ifndef DCTZ_CONTAINER_H
#define DCTZ_CONTAINER_H

#include <limits.h>
#include <stdint.h>
#include <string.h>

#include "dctz.h"

#define DZC_HEADER_BYTES 56
#define DZC_BINDEX_COUNT_OFF 52           /* header.bindex_count (QT) */
#define DZC_ND_BYTES 16                   /* "DZND" + three 32-bit extents */
#define DZC_IX_HEADER_BYTES 20            /* "DZIX", chunk bytes, chunks of section 0, 1, 2; then 16 bits per chunk */
#define DZC_UNKNOWN ((size_t)-1)          /* size of a container the caller cannot bound (dctz.h:127) */
typedef char dzc_header_is_56_bytes[sizeof(struct header) == DZC_HEADER_BYTES ? 1 : -1];

/* the buffer of a t_var as bytes */
static inline unsigned char *var_bytes(const t_var *v) { return v->datatype == DOUBLE ? (unsigned char *)v->buf.d : (unsigned char *)v->buf.f; }

/* ------------------------------------------------------------------------------------------------------ reading --- */
typedef struct {
  const unsigned char *z;                 /* the container */
  struct header h;                        /* copy of its header (bindex_count: see below) */
  t_datatype base;                        /* header.datatype without the geometry bits */
  int is_d;                               /* the type the view reads the container with (dzc_header) */
  size_t ts;                              /* bytes per element */
  int nd;                                 /* 0: the reference's flat blocks; else the geometry bits (sound: 2, 3) */
  size_t dims[3];
  size_t n, nblk, npos;                   /* elements; blocks; positions the streams cover (nd: edge tiles are padded) */
  unsigned int cnt, bindex_count;         /* tot_AC_exact_count; QT's count of bin ids (0 in an EC view) */
  double sf;
  size_t off[3];                          /* the sections: offset, compressed bytes, bytes they inflate to */
  const unsigned char *sec[3];
  unsigned int zlen[3];
  size_t raw[3];
  const unsigned char *qtable;            /* QT: the table (unaligned, in the data type); EC: NULL */
  size_t nd_off, ix_off;                  /* "DZND" (where it would be); end of what the header describes = where "DZIX" starts */
} dzc_view;

static inline void dzc_set_blocks(dzc_view *v, size_t nblk, size_t npos) {
  v->nblk = nblk; v->npos = npos;
  v->raw[0] = npos * sizeof(t_bin_id); v->raw[1] = nblk * sizeof(float); v->raw[2] = (size_t)v->cnt * sizeof(float);
}

/* Everything the 56 header bytes say (nothing else is read; no field is judged): a complete view of a flat container.
 * type: the element type to read it with -- the caller's tag, which is what the reference's reader follows
 * (var_z->datatype, dctz-decomp-lib.c:85-100), or DZC_TYPE_IN_HEADER. */
#define DZC_TYPE_IN_HEADER (-1)
static inline void dzc_header(dzc_view *v, const void *z, int qt, int type) {
  memset(v, 0, sizeof(*v));
  v->z = (const unsigned char *)z;
  memcpy(&v->h, z, sizeof(v->h));                                   /* dctz-decomp-lib.c:84-94 */
  if (qt) memcpy(&v->bindex_count, v->z + DZC_BINDEX_COUNT_OFF, sizeof(v->bindex_count));
  v->base = DCTZ_TYPE_OF(v->h.datatype);
  v->is_d = (type == DZC_TYPE_IN_HEADER ? (int)v->base : type) == DOUBLE;
  v->ts = v->is_d ? sizeof(double) : sizeof(float);
  v->nd = (int)DCTZ_GEOM_OF(v->h.datatype);
  v->n = v->h.num_elements;
  v->cnt = v->h.tot_AC_exact_count;
  v->sf = v->is_d ? v->h.scaling_factor.d : (double)v->h.scaling_factor.f;
  v->zlen[0] = v->h.bindex_sz_compressed; v->zlen[1] = v->h.DC_sz_compressed; v->zlen[2] = v->h.AC_exact_sz_compressed;
  size_t at = DZC_HEADER_BYTES;
  for (int i = 0; i < 3; i++) { v->off[i] = at; v->sec[i] = v->z + at; at += v->zlen[i]; }
  if (qt) { v->qtable = v->z + at; at += BLK_SZ * v->ts; }       /* :193-199 */
  v->nd_off = at;
  if (v->nd) at += DZC_ND_BYTES;
  v->ix_off = at;
  dzc_set_blocks(v, CEIL(v->n, BLK_SZ), v->n);
}

/* The extents of a multi-dimensional container (read at nd_off) -> dims, nblk (8 x 8 / 4 x 4 x 4 tiles), npos, raw.
 * Returns 0; 1: no "DZND" there (the view stays flat); 2: extents that are no shape the kernels take (what
 * dctzhip_nd_blocks refuses) or do not multiply to N -- the counts are then only good for printing. */
static inline int dzc_geometry(dzc_view *v) {
  unsigned int tr[4];
  memcpy(tr, v->z + v->nd_off, sizeof(tr));
  if (tr[0] != DCTZ_ND_MAGIC) return 1;
  const size_t edge = v->nd == 2 ? 8 : 4;
  size_t nblk = 1, prod = 1;
  int sound = v->nd == 2 || v->nd == 3;
  for (int i = 0; i < 3; i++) {
    v->dims[i] = tr[1 + i];
    if (i >= v->nd) continue;
    const size_t nb = (v->dims[i] + edge - 1) / edge;
    if (nb == 0 || v->dims[i] > (size_t)INT_MAX || nblk > (size_t)INT_MAX / BLK_SZ / nb) sound = 0;   /* nblk * 64 must stay an int (dctz.h:126) */
    nblk *= nb; prod *= v->dims[i];
  }
  dzc_set_blocks(v, nblk, nblk * BLK_SZ);
  return sound && prod == v->n ? 0 : 2;
}

/* The container in var_z: header + geometry, trusting the header as dctz_decompress must (it is not told the buffer's
 * size, dctz.h:127); nonzero: a bad multi-dimensional container */
static inline int dzc_open(dzc_view *v, const t_var *var_z, int qt) {
  dzc_header(v, var_bytes(var_z), qt, (int)var_z->datatype);
  return v->nd ? dzc_geometry(v) : 0;
}

/* the table as the kernels take it: copied out of the container (aligned); NULL in EC */
static inline const void *dzc_qtable(const dzc_view *v, double buf[BLK_SZ]) {
  if (!v->qtable) return NULL;
  memcpy(buf, v->qtable, BLK_SZ * v->ts);
  return buf;
}

static inline size_t dzc_index_bytes(size_t n0, size_t n1, size_t n2) { return (DZC_IX_HEADER_BYTES + 2 * (n0 + n1 + n2) + 3) & ~(size_t)3; }

/* The chunk index ("DZIX") as three arrays of compressed sizes (malloc; the caller frees them).
 *   DZC_IX_OK        the sections carry the mark (78 5E), the trailer is there and describes them exactly: chunk counts that
 *                    follow from the raw sizes, sizes that tile every stream up to its 03 00 + adler32
 *   DZC_IX_UNMARKED  ordinary zlib sections: nothing behind the container was looked at
 *   DZC_IX_BAD       marked, but the trailer is not an index of these sections
 *   DZC_IX_CUT       marked, and the index does not fit into zbytes (never with DZC_UNKNOWN)
 * Anything but DZC_IX_OK: nothing allocated, the reader takes the ordinary inflate. */
enum { DZC_IX_OK = 1, DZC_IX_UNMARKED = 0, DZC_IX_BAD = -1, DZC_IX_CUT = -2 };
static inline int dzc_read_index(const dzc_view *v, size_t zbytes, size_t *chunk_out, uint32_t *sizes[3]) {
  for (int i = 0; i < 3; i++) sizes[i] = NULL;
  for (int i = 0; i < 3; i++) if (v->zlen[i] < 8 || v->sec[i][0] != 0x78 || v->sec[i][1] != 0x5E) return DZC_IX_UNMARKED;
  if (zbytes < v->ix_off + DZC_IX_HEADER_BYTES) return DZC_IX_CUT;
  unsigned int hd[5];
  memcpy(hd, v->z + v->ix_off, sizeof(hd));
  if (hd[0] != DCTZ_IX_MAGIC || hd[1] < 1024 || hd[1] > 65535) return DZC_IX_BAD;
  const size_t chunk = hd[1];
  size_t entries = 0;
  for (int i = 0; i < 3; i++) { if (hd[2 + i] != (v->raw[i] + chunk - 1) / chunk) return DZC_IX_BAD; entries += hd[2 + i]; }
  if (zbytes < v->ix_off + DZC_IX_HEADER_BYTES + 2 * entries) return DZC_IX_CUT;
  const unsigned char *e = v->z + v->ix_off + DZC_IX_HEADER_BYTES;
  int ok = 1;
  for (int i = 0; i < 3 && ok; i++) {
    sizes[i] = (uint32_t *)malloc((hd[2 + i] ? hd[2 + i] : 1) * sizeof(uint32_t));
    if (!sizes[i]) { ok = 0; break; }
    size_t off = 2;
    for (size_t j = 0; j < hd[2 + i]; j++, e += 2) { unsigned short z; memcpy(&z, e, 2); sizes[i][j] = z; off += z; }
    if (off + 6 != v->zlen[i] || v->sec[i][off] != 0x03 || v->sec[i][off + 1] != 0x00) ok = 0;      /* the sizes must tile the stream */
  }
  if (!ok) { for (int i = 0; i < 3; i++) { free(sizes[i]); sizes[i] = NULL; } return DZC_IX_BAD; }
  *chunk_out = chunk;
  return DZC_IX_OK;
}

/* ------------------------------------------------------------------------------------------------------ writing --- */
/* What a writer knows once its three sections lie behind the header (dzc_sections), one after the other. */
typedef struct {
  t_datatype type;                        /* the caller's tag, as given */
  int nd;                                 /* multi-dimensional blocks: 2 / 3 and the extents; else 0 */
  const size_t *dims;
  size_t n, npos;
  double error_bound, sf, mean;           /* sf, mean: narrowed to fp32 in a FLOAT container */
  unsigned int cnt;
  size_t zlen[3];
  const double *qtable;                   /* QT: the 64 entries (written in the data type); EC: NULL */
  size_t chunk;                           /* "DZIX": chunk bytes, chunks and their compressed sizes per section; ix NULL: none */
  const size_t *ix_n;
  uint32_t *const *ix;
} dzc_desc;

static inline unsigned char *dzc_sections(unsigned char *z) { return z + DZC_HEADER_BYTES; }

/* Writes the header and everything behind the sections (dctz-comp-lib.c:775-820, then the trailers); returns the
 * container's size. */
static inline size_t dzc_finish(unsigned char *z, const dzc_desc *d) {
  const int is_d = d->type == DOUBLE;
  struct header h;
  memset(&h, 0, sizeof(h));
  h.datatype = (t_datatype)((unsigned)d->type | ((unsigned)d->nd << DCTZ_GEOM_SHIFT));
  h.num_elements = (unsigned int)d->n;
  h.error_bound = d->error_bound;
  h.tot_AC_exact_count = d->cnt;
  if (is_d) { h.scaling_factor.d = d->sf; h.mean.d = d->mean; }
  else { h.scaling_factor.f = (float)d->sf; h.mean.f = (float)d->mean; }
  h.bindex_sz_compressed = (unsigned int)d->zlen[0];
  h.DC_sz_compressed = (unsigned int)d->zlen[1];
  h.AC_exact_sz_compressed = (unsigned int)d->zlen[2];
  memcpy(z, &h, sizeof(h));
  unsigned char *cur = dzc_sections(z) + d->zlen[0] + d->zlen[1] + d->zlen[2];
  if (d->qtable) {
    const unsigned int bindex_count = (unsigned int)d->npos;        /* :798 */
    memcpy(z + DZC_BINDEX_COUNT_OFF, &bindex_count, sizeof(bindex_count));
    if (is_d) memcpy(cur, d->qtable, BLK_SZ * sizeof(double));
    else { float q[BLK_SZ]; for (int j = 0; j < BLK_SZ; j++) q[j] = (float)d->qtable[j]; memcpy(cur, q, sizeof(q)); }
    cur += BLK_SZ * (is_d ? sizeof(double) : sizeof(float));
  }
  if (d->nd) {
    const unsigned int tr[4] = {DCTZ_ND_MAGIC, (unsigned int)d->dims[0], (unsigned int)d->dims[1], (unsigned int)(d->nd == 3 ? d->dims[2] : 0)};
    memcpy(cur, tr, sizeof(tr));
    cur += sizeof(tr);
  }
  if (d->ix) {
    const unsigned int hd[5] = {DCTZ_IX_MAGIC, (unsigned int)d->chunk, (unsigned int)d->ix_n[0], (unsigned int)d->ix_n[1], (unsigned int)d->ix_n[2]};
    const size_t ix_bytes = dzc_index_bytes(d->ix_n[0], d->ix_n[1], d->ix_n[2]);
    memset(cur, 0, ix_bytes);
    memcpy(cur, hd, sizeof(hd));
    unsigned char *e = cur + sizeof(hd);
    for (int i = 0; i < 3; i++)
      for (size_t k = 0; k < d->ix_n[i]; k++, e += 2) { const unsigned short s = (unsigned short)d->ix[i][k]; memcpy(e, &s, 2); }
    cur += ix_bytes;
  }
  return (size_t)(cur - z);
}

#endif /* DCTZ_CONTAINER_H */
