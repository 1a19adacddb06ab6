// The library's counter-based generator, Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11),
// shared by the dropout masks (dropout.hip) and the LR-only augmentations (augment.hip).  tests/philox_ref.py restates it in
// numpy and pins it to Random123's known-answer vectors.
#pragma once
#include "common.h"

// Philox4x32-10 of counter (c0, c1, c2, 0) under key (k0, k1)
__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1) {
  unsigned c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return uint4{c0, c1, c2, c3};
}
