// Prints what dctz_quant_host.h (the quantiser's launch constants, host only) computes, for tests/test_quant_host_cpu.py to
// compare bit for bit with its numpy restatement.  Stand-alone: built with -fsanitize=address,undefined by that test.
// One request per argument, fields separated by ':', every double as the 16 hex digits of its bit pattern; one line of
// output per request, values of the element type as the hex digits of THEIR bit pattern (8 for f32):
//   q:<f32|f64>:<eb>:<fastdiv>                       -> fwd bin_width range_min range_max fast_bw, inv bin_width range_min range_max
//   l:<f32|f64>:<max_abs>:<min_abs>:<fastdiv>        -> fast_sf_level for sf = scaling_factor(max_abs) in the element type, true statistics;
//                                                       the same with placeholder statistics
//   v:<f32|f64>:<max_abs>:<min_abs>:<sf_used>:<fast_used> -> device_sf_stands, true_sf
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dctz_quant_host.h"

using namespace dctz;

static double dbl(const std::string& s) {
  const uint64_t b = std::strtoull(s.c_str(), nullptr, 16);
  double v;
  std::memcpy(&v, &b, sizeof(v));
  return v;
}
static uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, sizeof(v)); return b; }
static uint64_t bits(float v) { uint32_t b; std::memcpy(&b, &v, sizeof(v)); return b; }

template <typename T>
static void constants(double eb, int fastdiv) {
  const FwdQuant<T> f = fwd_quant<T>(eb, fastdiv);
  const InvQuant<T> i = inv_quant<T>(eb);
  std::printf("%" PRIx64 " %" PRIx64 " %" PRIx64 " %u %" PRIx64 " %" PRIx64 " %" PRIx64 "\n", bits(f.bin_width), bits(f.range_min), bits(f.range_max),
              f.fast_bw, bits(i.bin_width), bits(i.range_min), bits(i.range_max));
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    std::vector<std::string> f;
    for (const char* p = argv[a];;) {
      const char* e = std::strchr(p, ':');
      f.push_back(e ? std::string(p, e) : std::string(p));
      if (!e) break;
      p = e + 1;
    }
    const size_t want = f[0] == "q" ? 4 : f[0] == "l" ? 5 : f[0] == "v" ? 6 : 0;
    if (!want || f.size() != want || (f[1] != "f32" && f[1] != "f64")) { std::printf("bad request %s\n", argv[a]); return 2; }
    const int dtype = f[1] == "f64" ? DCTZHIP_F64 : DCTZHIP_F32;
    if (f[0] == "q") {
      if (dtype == DCTZHIP_F64) constants<double>(dbl(f[2]), std::atoi(f[3].c_str()));
      else constants<float>(dbl(f[2]), std::atoi(f[3].c_str()));
    } else if (f[0] == "l") {
      const double mx = dbl(f[2]), mn = dbl(f[3]), sf = scaling_factor(dtype, mx);
      const double sf_in_t = dtype == DCTZHIP_F64 ? sf : (double)(float)sf;
      const int fastdiv = std::atoi(f[4].c_str());
      std::printf("%u %u\n", fast_sf_level(dtype, fastdiv, sf_in_t, mn, mx, true), fast_sf_level(dtype, fastdiv, sf_in_t, mn, mx, false));
    } else {
      double true_sf = -1.0;
      const bool ok = device_sf_stands(dtype, dbl(f[2]), dbl(f[3]), dbl(f[4]), (unsigned)std::atoi(f[5].c_str()), &true_sf);
      std::printf("%d %" PRIx64 "\n", ok ? 1 : 0, bits(true_sf));
    }
  }
  return 0;
}
