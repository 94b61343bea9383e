// philox.hip.h -- the counter RNG of the sampling kernels (sampling_kernels.hip, ray_batch_kernels.hip): one definition, so that a ray
// batch draws the bits an image render draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Philox-4x32-10, key = seed, counter = (pixel_index, stream, k/4, 0); same stream as the CPU oracle.
__device__ __forceinline__ void philox4x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                           uint32_t c3, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 9) * (1.0f / 8388608.0f); }

} // namespace
