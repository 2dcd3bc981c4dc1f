/*
 * dctz_mask_blob.h -- the layout of a missing-value mask blob, in one place (internal; what it means: include/dctz_hip.h,
 * "missing values"; who makes and reads it: dctz_compress_masked / dctz_decompress_masked in include/dctz.h):
 *
 *   header (48 bytes) | payload
 *
 *   header     "DZMK", version (1), dtype (t_datatype of the array), flags (the DCTZHIP_MISS_* tests that made the mask), n,
 *              count (the missing elements), fill (double: what a decode writes into them), words = ceil(n / 64), payload
 *              bytes; host byte order like the .z container
 *   payload    the `words` 64-bit mask words as ONE zlib stream (compress2, level 6)
 * The blob lives beside the container, never in it: the .z layout does not know it.
 */
#ifndef DCTZ_MASK_BLOB_H
#define DCTZ_MASK_BLOB_H

#include <stdint.h>
#include <string.h>

#define DZMK_MAGIC "DZMK"
#define DZMK_VERSION 1u
#define DZMK_HEADER_BYTES 48
#define DZMK_ZLIB_LEVEL 6
#define DZMK_FLAGS_ALL 15u

typedef struct {
  char magic[4];
  uint32_t version, dtype, flags;
  uint64_t n, count;
  double fill;
  uint32_t words, payload_bytes;
} dzmk_header;
typedef char dzmk_header_is_48_bytes[sizeof(dzmk_header) == DZMK_HEADER_BYTES ? 1 : -1];

static inline void dzmk_write_header(void *blob, int is_d, unsigned flags, size_t n, size_t count, double fill, size_t payload_bytes) {
  dzmk_header h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, DZMK_MAGIC, 4);
  h.version = DZMK_VERSION;
  h.dtype = (uint32_t)is_d;
  h.flags = flags;
  h.n = n; h.count = count;
  h.fill = fill;
  h.words = (uint32_t)((n + 63) / 64); h.payload_bytes = (uint32_t)payload_bytes;
  memcpy(blob, &h, sizeof(h));
}

/* The header of a blob against the array it is meant for (is_d, n elements): 0 and *h filled, or -1 for a blob too short for
 * its header, a wrong magic, version or dtype, flags that name no test or an unknown one, another n, a word count or a count
 * that cannot be this array's, an empty payload, or a length that is not the one the header describes.  Only the header is
 * read. */
static inline int dzmk_check(const void *blob, size_t blob_bytes, int is_d, size_t n, dzmk_header *h) {
  if (!blob || blob_bytes < DZMK_HEADER_BYTES) return -1;
  memcpy(h, blob, sizeof(*h));
  if (memcmp(h->magic, DZMK_MAGIC, 4) != 0 || h->version != DZMK_VERSION) return -1;
  if (h->dtype != (uint32_t)(is_d != 0) || h->flags == 0 || (h->flags & ~DZMK_FLAGS_ALL)) return -1;
  if (h->n != n || h->words != (n + 63) / 64 || h->count > n) return -1;
  if (h->payload_bytes == 0 || blob_bytes != (size_t)DZMK_HEADER_BYTES + h->payload_bytes) return -1;
  return 0;
}

#endif /* DCTZ_MASK_BLOB_H */
