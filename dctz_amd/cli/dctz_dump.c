/* dctz_dump.c -- inspect a DCTZ container.
 *
 *   dctz-dump <file.z>            the reference tool's six lines (tools/dctz-dump.c:41-50)
 *   dctz-dump -v <file.z>         + section sizes, offsets, a bounds check of the whole layout
 *                                   against the file size, and (QT files) the table's first entries
 *
 * The header is `struct header` of dctz.h:96-119: 56 bytes, native little-endian, then
 * deflate(bin_index[N]) | deflate(DC[nblk] as float) | deflate(AC_exact[cnt] as float)
 * [| qtable[64] in the data type]  (dctz-comp-lib.c:775-820).  EC and QT headers have the
 * same size (the QT-only bindex_count sits in what is padding in the EC layout), so one
 * binary reads both; -v tells them apart by the file size.  The layout itself is csrc/dctz_container.h's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../csrc/dctz_container.h"

int main(int argc, char *argv[]) {
  int verbose = 0;
  const char *path = NULL;
  if (argc == 2) path = argv[1];
  else if (argc == 3 && strcmp(argv[1], "-v") == 0) { verbose = 1; path = argv[2]; }
  if (!path) {
    printf("Usage: %s filename\n", argv[0]);
    exit(0);
  }
  FILE *fp = fopen(path, "rb");
  if (!fp) {
    perror("Failed: ");
    printf("File Not Found\n");
    return 0;
  }
  fseek(fp, 0, SEEK_END);
  const long fsz_all = ftell(fp);
  rewind(fp);
  unsigned char *buf = (unsigned char *)malloc(fsz_all > 0 ? (size_t)fsz_all : 1);
  if (fsz_all < DZC_HEADER_BYTES || !buf || fread(buf, (size_t)fsz_all, 1, fp) != 1) {
    printf("%s: shorter than a DCTZ header (%zu bytes)\n", path, (size_t)DZC_HEADER_BYTES);
    fclose(fp);
    return 1;
  }
  fclose(fp);
  dzc_view ec, qt;                                          /* the file read as either variant (qt: bindex_count, the table) */
  dzc_header(&ec, buf, 0, DZC_TYPE_IN_HEADER);
  dzc_header(&qt, buf, 1, DZC_TYPE_IN_HEADER);
  const struct header *h = &ec.h;
  printf("File Name=%s\n", path);
  printf("data type=%s\n", ec.is_d ? "double" : "float");
  printf("N=%d\n", h->num_elements);
  printf("error_bound=%f\n", h->error_bound);
  printf("total # of AC_exact=%d\n", h->tot_AC_exact_count);
  printf("SF=%f\n", ec.sf);

  int rc = 0;
  if (verbose) {
    const unsigned geom = (unsigned)ec.nd;                  /* 0: the reference's flat blocks; 2, 3: tiles (dctz.h) */
    const size_t ts = ec.ts;
    /* "DZIX" chunk index behind everything else (written when the entropy stage ran on the GPU, dctz.h): look where an
     * ec and where a qt container would have it */
    long ix_bytes = 0;
    unsigned int ixh[5] = {0, 0, 0, 0, 0};
    for (int q = 0; q < 2 && !ix_bytes; q++) {
      const size_t pos = q ? qt.ix_off : ec.ix_off;
      if (pos + DZC_IX_HEADER_BYTES > (size_t)fsz_all) continue;
      memcpy(ixh, buf + pos, sizeof(ixh));
      if (ixh[0] == DCTZ_IX_MAGIC && pos + dzc_index_bytes(ixh[2], ixh[3], ixh[4]) == (size_t)fsz_all) ix_bytes = fsz_all - (long)pos;
    }
    const long fsz = fsz_all - ix_bytes;
    if (geom) {                                             /* "DZND" + three extents close the file */
      ec.nd_off = (size_t)fsz - DZC_ND_BYTES;               /* (look there even when the header's sizes do not add up to it) */
      if (fsz >= DZC_ND_BYTES && dzc_geometry(&ec) != 1) {
        if (geom == 2) printf("multi-dimensional blocks: %zu x %zu array, 8 x 8 tiles\n", ec.dims[0], ec.dims[1]);
        else printf("multi-dimensional blocks: %zu x %zu x %zu array, 4 x 4 x 4 tiles\n", ec.dims[0], ec.dims[1], ec.dims[2]);
      } else {
        printf("LAYOUT MISMATCH: geometry %u in the header but no extents at the end of the file\n", geom);
        rc = 2;
      }
    }
    printf("mean=%.17g\n", ec.is_d ? h->mean.d : (double)h->mean.f);
    printf("blocks=%zu (last one %zu elements)\n", ec.nblk, (!geom && h->num_elements % BLK_SZ) ? (size_t)(h->num_elements % BLK_SZ) : (size_t)BLK_SZ);
    printf("bin_index: offset %zu, %u bytes deflated (%zu raw)\n", ec.off[0], ec.zlen[0], ec.raw[0]);
    printf("DC:        offset %zu, %u bytes deflated (%zu raw)\n", ec.off[1], ec.zlen[1], ec.raw[1]);
    printf("AC_exact:  offset %zu, %u bytes deflated (%zu raw)\n", ec.off[2], ec.zlen[2], ec.raw[2]);
    if ((size_t)fsz == ec.ix_off) {
      printf("variant=ec (no table), file size %ld = layout\n", fsz);
    } else if ((size_t)fsz == qt.ix_off) {
      printf("variant=qt, bindex_count=%u, table at offset %zu, file size %ld = layout\n", qt.bindex_count, (size_t)(qt.qtable - buf), fsz);
      printf("qtable[1..4]=");
      for (int j = 1; j <= 4; j++) {
        double v;
        if (ts == 8) memcpy(&v, qt.qtable + 8 * j, 8);
        else { float f; memcpy(&f, qt.qtable + 4 * j, 4); v = f; }
        printf("%s%.9g", j > 1 ? ", " : "", v);
      }
      printf("\n");
    } else {
      printf("LAYOUT MISMATCH: header describes %zu bytes (ec) or %zu (qt), file has %ld\n", ec.ix_off, qt.ix_off, fsz);
      rc = 2;
    }
    if (ix_bytes) {
      printf("chunk index: %ld bytes at offset %ld, chunks of %u bytes: %u + %u + %u (sections made by the GPU entropy stage)\n", ix_bytes, fsz,
             ixh[1], ixh[2], ixh[3], ixh[4]);
      /* the sizes of a section's chunks + 2 (zlib header) + 6 (03 00 + adler32) must be the section's size */
      const unsigned char *e = buf + fsz + DZC_IX_HEADER_BYTES;
      int tiles = 1;
      for (int i = 0; i < 3; i++) {
        unsigned long long sum = 8;
        for (unsigned int k = 0; k < ixh[2 + i]; k++, e += 2) { unsigned short z; memcpy(&z, e, 2); sum += z; }
        if (sum != ec.zlen[i]) tiles = 0;
      }
      printf("chunk index %s\n", tiles ? "tiles the three streams" : "does NOT tile the streams");
      if (!tiles) rc = 2;
    }
    printf("compression ratio=%.2f\n", (double)h->num_elements * ts / (double)fsz_all);
  }
  free(buf);
  return rc;
}
