/*
 * dctz_fixup_blob.h -- the layout of a correction-list blob, in one place (internal; what it means: include/dctz_hip.h,
 * "point-wise error bound"; who makes and reads it: dctz_fixup_build / dctz_decompress_bounded in include/dctz.h):
 *
 *   header (48 bytes) | fix_start | fix_off | fix_val
 *
 *   header     "DZFX", version (1), dtype (t_datatype of the array), 4 bytes of zero, n, tiles = ceil(n / 4096), count (64 bits
 *              each), bound (double); host byte order like the .z container
 *   fix_start  tiles + 1 entries of 32 bits, padded with zeros to a multiple of 8 bytes
 *   fix_off    count entries of 16 bits, padded with zeros to a multiple of 8 bytes
 *   fix_val    count elements of the data type
 * The blob lives beside the container, never in it: the .z layout does not know it.
 *
 * The list of an array compressed in 8 x 8 / 4 x 4 x 4 tiles (a "DZND" container) is version 2:
 *
 *   header (72 bytes) | fix_start | fix_off | fix_val
 *
 *   header     the 48 bytes above with version 2, the zero field holding ndims (2 or 3), n = the product of the extents and
 *              tiles = ceil(64 nblk / 4096) over the nblk blocks of the tile grid; then the extents, 64 bits each, unused
 *              entries 0
 *   the three arrays as above: their offsets count from the end of the header.  fix_off holds stream positions modulo 4096
 *   (include/dctz_hip.h: dctzhip_fixup_build_nd).
 * A flat blob stays version 1, byte for byte.
 */
#ifndef DCTZ_FIXUP_BLOB_H
#define DCTZ_FIXUP_BLOB_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#define DZFX_MAGIC "DZFX"
#define DZFX_VERSION 1u
#define DZFX_HEADER_BYTES 48
#define DZFX_TILE 4096
#define DZFX_VERSION_ND 2u
#define DZFX_HEADER_BYTES_ND 72

typedef struct {
  char magic[4];
  uint32_t version, dtype, zero;
  uint64_t n, tiles, count;
  double bound;
} dzfx_header;
typedef char dzfx_header_is_48_bytes[sizeof(dzfx_header) == DZFX_HEADER_BYTES ? 1 : -1];

static inline size_t dzfx_pad8(size_t v) { return (v + 7) & ~(size_t)7; }
/* offsets of the three arrays behind the header, and the size of the payload */
static inline size_t dzfx_off_at(size_t tiles) { return dzfx_pad8((tiles + 1) * sizeof(uint32_t)); }
static inline size_t dzfx_val_at(size_t tiles, size_t count) { return dzfx_off_at(tiles) + dzfx_pad8(count * sizeof(uint16_t)); }
static inline size_t dzfx_payload_bytes(size_t tiles, size_t count, size_t ts) { return dzfx_val_at(tiles, count) + count * ts; }
/* the three arrays of a payload that starts at p, in host or device memory alike */
typedef struct { uint32_t *start; uint16_t *off; void *val; } dzfx_arrays;
static inline dzfx_arrays dzfx_arrays_at(void *p, size_t tiles, size_t count) {
  unsigned char *const d = (unsigned char *)p;
  const dzfx_arrays a = {(uint32_t *)d, (uint16_t *)(d + dzfx_off_at(tiles)), d + dzfx_val_at(tiles, count)};
  return a;
}

static inline void dzfx_write_header(void *blob, int is_d, size_t n, size_t count, double bound) {
  dzfx_header h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, DZFX_MAGIC, 4);
  h.version = DZFX_VERSION;
  h.dtype = (uint32_t)is_d;
  h.n = n; h.tiles = (n + DZFX_TILE - 1) / DZFX_TILE; h.count = count;
  h.bound = bound;
  memcpy(blob, &h, sizeof(h));
}

/* The header of a blob against the array it is meant for (is_d, n elements): 0 and *h filled, or -1 for a blob too short for
 * its header, a wrong magic, version or dtype, another n, a tile count or a count that cannot be this array's, a bound that
 * is none, or a length that is not the one the header describes.  Only the header is read. */
static inline int dzfx_check(const void *blob, size_t blob_bytes, int is_d, size_t n, dzfx_header *h) {
  if (!blob || blob_bytes < DZFX_HEADER_BYTES) return -1;
  memcpy(h, blob, sizeof(*h));
  if (memcmp(h->magic, DZFX_MAGIC, 4) != 0 || h->version != DZFX_VERSION) return -1;
  if (h->dtype != (uint32_t)(is_d != 0) || h->zero != 0) return -1;
  if (h->n != n || h->tiles != (n + DZFX_TILE - 1) / DZFX_TILE || h->count > n) return -1;
  if (!(h->bound >= 0.0) || isinf(h->bound)) return -1;
  if (blob_bytes != DZFX_HEADER_BYTES + dzfx_payload_bytes((size_t)h->tiles, (size_t)h->count, is_d ? sizeof(double) : sizeof(float))) return -1;
  return 0;
}

/* ---- version 2: tiled arrays ---- */
typedef struct {
  dzfx_header h;                          /* h.zero = ndims */
  uint64_t dims[3];
} dzfx_header_nd;
typedef char dzfx_header_nd_is_72_bytes[sizeof(dzfx_header_nd) == DZFX_HEADER_BYTES_ND ? 1 : -1];

/* what a blob's header says about itself: its version (0: too short to say) and where its arrays start */
static inline uint32_t dzfx_version(const void *blob, size_t blob_bytes) {
  dzfx_header h;
  if (!blob || blob_bytes < DZFX_HEADER_BYTES) return 0;
  memcpy(&h, blob, sizeof(h));
  return h.version;
}
static inline size_t dzfx_header_bytes(uint32_t version) { return version == DZFX_VERSION_ND ? DZFX_HEADER_BYTES_ND : DZFX_HEADER_BYTES; }
static inline size_t dzfx_tiles_nd(size_t nblk) { return (nblk * 64 + DZFX_TILE - 1) / DZFX_TILE; }

static inline void dzfx_write_header_nd(void *blob, int is_d, int nd, const size_t *dims, size_t n, size_t nblk, size_t count, double bound) {
  dzfx_header_nd h;
  memset(&h, 0, sizeof(h));
  memcpy(h.h.magic, DZFX_MAGIC, 4);
  h.h.version = DZFX_VERSION_ND;
  h.h.dtype = (uint32_t)is_d;
  h.h.zero = (uint32_t)nd;
  h.h.n = n; h.h.tiles = dzfx_tiles_nd(nblk); h.h.count = count;
  h.h.bound = bound;
  for (int i = 0; i < nd && i < 3; i++) h.dims[i] = dims[i];
  memcpy(blob, &h, sizeof(h));
}

/* dzfx_check for a version-2 blob against the tiled array it is meant for (is_d, nd extents dims, n = their product, nblk
 * blocks): 0 and *h filled, or -1 for what dzfx_check refuses, another ndims, other extents (100 x 200 against 200 x 100), and
 * a count above the real positions.  Only the header is read. */
static inline int dzfx_check_nd(const void *blob, size_t blob_bytes, int is_d, int nd, const size_t *dims, size_t n, size_t nblk, dzfx_header_nd *h) {
  if (!blob || blob_bytes < DZFX_HEADER_BYTES_ND || (nd != 2 && nd != 3)) return -1;
  memcpy(h, blob, sizeof(*h));
  if (memcmp(h->h.magic, DZFX_MAGIC, 4) != 0 || h->h.version != DZFX_VERSION_ND) return -1;
  if (h->h.dtype != (uint32_t)(is_d != 0) || h->h.zero != (uint32_t)nd) return -1;
  for (int i = 0; i < 3; i++) if (h->dims[i] != (i < nd ? (uint64_t)dims[i] : 0u)) return -1;
  if (h->h.n != n || h->h.tiles != dzfx_tiles_nd(nblk) || h->h.count > n) return -1;
  if (!(h->h.bound >= 0.0) || isinf(h->h.bound)) return -1;
  if (blob_bytes != DZFX_HEADER_BYTES_ND + dzfx_payload_bytes((size_t)h->h.tiles, (size_t)h->h.count, is_d ? sizeof(double) : sizeof(float))) return -1;
  return 0;
}

#endif /* DCTZ_FIXUP_BLOB_H */
