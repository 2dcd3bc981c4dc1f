// emu_lowband.cpp -- TEST HARNESS: runs the PRODUCT's low-band inverse transforms (dctz_amd/csrc/dct_lowband_block.h, the
// code one GPU lane executes in the coarse decoders) on the CPU.  Build: g++ -O1 -ffp-contract=off -mfma -shared -fPIC
// (tests/test_lowband_header.py).
#include "../../dctz_amd/csrc/dct_lowband_block.h"

using namespace dctz;

template <typename T, int N, int K>
static void flat(const T* c, T* y) {
  T a[K], b[K];
  for (int i = 0; i < K; i++) a[i] = c[i];
  lowband_inv<T, N, K>(a, b);
  for (int i = 0; i < K; i++) y[i] = b[i];
}
template <typename T>
static int flat_k(int n, int k, const T* c, T* y) {
  if (n == 64) {
    switch (k) {
      case 1: flat<T, 64, 1>(c, y); return 0;
      case 2: flat<T, 64, 2>(c, y); return 0;
      case 4: flat<T, 64, 4>(c, y); return 0;
      case 8: flat<T, 64, 8>(c, y); return 0;
      case 16: flat<T, 64, 16>(c, y); return 0;
      case 32: flat<T, 64, 32>(c, y); return 0;
    }
  } else if (n == 8) {
    switch (k) {
      case 1: flat<T, 8, 1>(c, y); return 0;
      case 2: flat<T, 8, 2>(c, y); return 0;
      case 4: flat<T, 8, 4>(c, y); return 0;
    }
  } else if (n == 4) {
    switch (k) {
      case 1: flat<T, 4, 1>(c, y); return 0;
      case 2: flat<T, 4, 2>(c, y); return 0;
    }
  }
  return -1;
}
// geom 1: the K x K corner of an 8 x 8 tile (K = 2 | 4); geom 2: the 2 x 2 x 2 corner of a 4 x 4 x 4 tile; in place
template <typename T>
static int tile_k(int geom, int k, T* v) {
  if (geom == 1 && k == 2) { T a[4]; for (int i = 0; i < 4; i++) a[i] = v[i]; lowband_inv_2d<T, 2>(a); for (int i = 0; i < 4; i++) v[i] = a[i]; return 0; }
  if (geom == 1 && k == 4) { T a[16]; for (int i = 0; i < 16; i++) a[i] = v[i]; lowband_inv_2d<T, 4>(a); for (int i = 0; i < 16; i++) v[i] = a[i]; return 0; }
  if (geom == 2 && k == 2) { T a[8]; for (int i = 0; i < 8; i++) a[i] = v[i]; lowband_inv_3d<T, 2>(a); for (int i = 0; i < 8; i++) v[i] = a[i]; return 0; }
  return -1;
}

extern "C" {
int emu_lowband_f64(int n, int k, const double* c, double* y) { return flat_k<double>(n, k, c, y); }
int emu_lowband_f32(int n, int k, const float* c, float* y) { return flat_k<float>(n, k, c, y); }
int emu_lowband_tile_f64(int geom, int k, double* v) { return tile_k<double>(geom, k, v); }
int emu_lowband_tile_f32(int geom, int k, float* v) { return tile_k<float>(geom, k, v); }
double emu_lowband_cos(int m) { return lb_cos<double>(m); }
}
