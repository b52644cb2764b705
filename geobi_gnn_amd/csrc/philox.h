// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and the
// word -> uniform map, shared by noise.hip and sample.hip.  Counter layout of every user: (row, stream_id, draw, block),
// key = (seed & 0xffffffff, seed >> 32).  The blocks in use: 0 and 1 noise.hip, 2 sample.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace geobi {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return U4{c0, c1, c2, c3};
}

// u = ((w >> 9) + 0.5) * 2^-23: exact in fp32, never 0 or 1
__device__ __forceinline__ float word_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

}  // namespace geobi
