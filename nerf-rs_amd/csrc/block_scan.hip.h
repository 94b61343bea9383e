// block_scan.hip.h -- the workgroup-level pieces of the deterministic compaction idiom (flags -> block sums -> one-workgroup scan ->
// scatter) that normal_kernels.hip, ray_clip_kernels.hip and surface_kernels.hip share.  Device code only; wave64, workgroups of
// kScanBlock = 256 threads (four waves).  `s` is kScanBlock / 64 words of LDS that the caller declares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kScanBlock = 256;

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// exclusive prefix sum of v over the kScanBlock threads of the workgroup; sum = the workgroup's total.  Ends with a barrier: s is free again.
__device__ __forceinline__ void block_exclusive(uint32_t &v, uint32_t &sum, uint32_t *s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t iv = wave_inclusive(v, lane);
    if (lane == 63) s[wave] = iv;
    __syncthreads();
    uint32_t ov = 0;
    sum = 0;
#pragma unroll
    for (int k = 0; k < kScanBlock / 64; ++k) {
        if (k < wave) ov += s[k];
        sum += s[k];
    }
    v = iv - v + ov;
    __syncthreads();
}

// the number of threads of the workgroup whose flag is set, in every thread.  One barrier: every thread of the workgroup must call it.
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t *s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = (uint32_t)__popcll(__ballot(flag));
    if (lane == 0) s[wave] = c;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanBlock / 64; ++k) sum += s[k];
    return sum;
}
