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

#endif /* DCTZ_FIXUP_BLOB_H */
