// dctz_nd_image.h -- the LDS image of a stream tile of an array compressed in 8 x 8 / 4 x 4 x 4 tiles, as the kernels that
// walk it in row strips lay it out (dctz_kernels_ndbox.hip: k_decompress_ndbox; dctz_kernels_ndfix.hip: k_ndfix_mark;
// dctz_kernels_ndsummary.hip: k_ndsummary), and the array coordinates of a stream position.
#pragma once
#include "dctz_kernel_common.h"

namespace dctz {

// Block b of the tile at elements [b * STRIDE, b * STRIDE + 64).  The read-back of step s, in-block row r has lane l at
// (l / e + 64 / e * s) * STRIDE + e r + l % e; the image is written by lane b's 16-byte stores at b * STRIDE + 4 | 2 ch.
//   fp32, 8 x 8 (ds_read_b32: 32 lanes per cycle, 32 banks): 4 blocks x 8 dwords -> STRIDE = 8 mod 32 is conflict-free
//     (72); the 16-byte writes (8 lanes per cycle, 32 banks) then pair up lanes b and b + 4: 16 array cycles for the 13 the
//     instruction takes anyway.  RaGeo's 68 would make every one of the 64 reads 2-way.
//   fp32, 4 x 4 x 4: 8 blocks x 4 dwords -> STRIDE = 4 mod 32: RaGeo's 68, conflict-free both ways.
//   fp64, 8 x 8 (ds_read_b64: 32 lanes, 64 banks): 4 blocks x 16 dwords -> conflict-free needs STRIDE = 8 mod 32, which
//     puts the writes of 8 lanes on 2 x 16 banks (4-way, 32 writes a tile).  70: writes conflict-free (12 b mod 32 takes
//     8 values 4 apart), reads 2-way.  RaGeo's 66 reads 4-way.
//   fp64, 4 x 4 x 4: 8 blocks x 8 dwords -> STRIDE = 4 mod 32 (68) reads conflict-free, writes 2-way (16 cycles for 13).
template <typename T, int GEOM> struct NdImage {
  static constexpr int EPV = Traits<T>::EPV;
  static constexpr int STRIDE = GEOM == GEOM_3D ? 68 : (sizeof(T) == 8 ? 70 : 72);
  static constexpr int BYTES = TILE_BLKS * STRIDE * (int)sizeof(T);
  static_assert(STRIDE % EPV == 0, "16-byte rows");
  static_assert(BYTES >= 63 * 64 * 4, "a dense tile's exact coefficients fit the image");
};

// The grid coordinates of block B (2-D: z = 0)
template <int GEOM>
__device__ __forceinline__ void ndfix_block(const unsigned B, const unsigned nbx, const unsigned nby, unsigned& bz, unsigned& by, unsigned& bx) {
  const unsigned q = B / nbx;
  bx = B - q * nbx;
  bz = GEOM == GEOM_3D ? q / nby : 0u;
  by = q - bz * nby;
}
// ... and the array coordinates of its in-block place j
template <int GEOM>
__device__ __forceinline__ void ndfix_place(const unsigned bz, const unsigned by, const unsigned bx, const unsigned j, unsigned& z, unsigned& y,
                                            unsigned& x) {
  if (GEOM == GEOM_3D) { z = bz * 4u + (j >> 4); y = by * 4u + ((j >> 2) & 3u); x = bx * 4u + (j & 3u); }
  else { z = 0u; y = by * 8u + (j >> 3); x = bx * 8u + (j & 7u); }
}

// bit j: in-block place j of block (bz, by, bx) lies inside the array
template <int GEOM>
__device__ __forceinline__ unsigned long long nd_real_mask(const unsigned bz, const unsigned by, const unsigned bx, const unsigned dz,
                                                           const unsigned dy, const unsigned dx) {
  if (GEOM == GEOM_3D) {
    const unsigned nx = min(4u, dx - bx * 4u), ny = min(4u, dy - by * 4u), nz = min(4u, dz - bz * 4u);
    const unsigned plane = (((1u << nx) - 1u) * 0x1111u) & ((1u << (4u * ny)) - 1u);
    const unsigned long long all = (unsigned long long)plane * 0x0001000100010001ull;
    return nz == 4u ? all : all & ((1ull << (16u * nz)) - 1ull);
  }
  const unsigned nx = min(8u, dx - bx * 8u), ny = min(8u, dy - by * 8u);
  const unsigned long long all = (unsigned long long)((1u << nx) - 1u) * 0x0101010101010101ull;
  return ny == 8u ? all : all & ((1ull << (8u * ny)) - 1ull);
}

}  // namespace dctz
