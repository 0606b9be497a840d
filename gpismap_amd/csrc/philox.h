// The counter generator of the particle filter and of the sampling controller: Philox4x32-10 and the
// integer sum-of-uniforms deviate of one block.  Stateless, host and device; this header is the one statement of both.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace gpis {

constexpr double kPhiloxKZ = 0x1.3988e1412ed76p-17;        // 1 / sqrt(8 (65536^2 - 1) / 3)

__host__ __device__ __forceinline__ void philox10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                  uint32_t* __restrict__ out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the deviate of the block of one counter: its eight 16-bit halves summed as integers, one conversion, one product
__device__ __forceinline__ double philox_deviate(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    uint32_t w[4];
    philox10(c0, c1, c2, c3, k0, k1, w);
    int S = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) S += (int)(w[a] & 0xFFFFu) + (int)(w[a] >> 16);
    return (double)(2 * S - 8 * 65535) * kPhiloxKZ;
}

}  // namespace gpis
