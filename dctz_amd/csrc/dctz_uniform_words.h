// dctz_uniform_words.h -- a record of a device table into scalar registers: what the list decoders of tiled arrays read per
// item (dctz_kernels_mboxnd.hip, dctz_kernels_mcboxnd.hip).
#pragma once

namespace dctz {

// word by word (every lane reads the same address)
template <typename R>
__device__ __forceinline__ R uniform_words(const R* r) {
  static_assert(sizeof(R) % 4 == 0, "read word by word");
  struct Words { unsigned w[sizeof(R) / 4]; } v;
  const unsigned* s = reinterpret_cast<const unsigned*>(r);
#pragma unroll
  for (unsigned i = 0; i < sizeof(R) / 4; i++) v.w[i] = (unsigned)__builtin_amdgcn_readfirstlane((int)s[i]);
  return __builtin_bit_cast(R, v);
}

}  // namespace dctz
