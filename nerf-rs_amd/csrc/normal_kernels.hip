// normal_kernels.hip -- central differences of sigma around caller points and around the live samples of a ray batch, and the per-ray
// normal they add up to.  The contract (every rounding) is in include/nerf_mi355x.h, "surface normals"; tests/helpers/normal_restatement.py
// restates it.  The densities themselves come from the f32 sigma-only MLP_MODE_POINTS launch between k_normal_stencil and
// k_normal_reduce / k_normal_combine; nothing here evaluates a network.
//
//   k_normal_block_sums  per ray the number of live samples (weight > 0), per 256 rays their sum
//   k_normal_scan_sums   ONE workgroup: exclusive prefix sums of the block sums in place, 256 at a time with a carry; the total
//   k_normal_scan_add    per ray the exclusive prefix sum of the counts + the block's offset -> base; the live sample indices -> list
//   k_normal_stencil     one thread per live sample (or caller point): its six stencil points, SoA
//   k_normal_reduce      one thread per ray: walks its live samples in order, accumulates w * g, normalises
//   k_normal_combine     one thread per caller point: g
// Every output position is fixed by prefix sums: no atomics, no kernel waits for another workgroup, the same bits in every run.
// Built like sampling_kernels.hip: IEEE f32 without contraction, correctly rounded divide and sqrt.  Wave64, 256-thread workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.hip.h"
#include "normal_kernels.h"

namespace {

constexpr int kB = kNormalBlock;
static_assert(kB == kScanBlock, "four waves of 64 rays per workgroup (block_scan.hip.h)");

// A wave owns 64 consecutive rays and visits them one after the other, its lanes striding over the ray's samples: the weight loads are
// contiguous.  Returns in lane j the number of live samples of ray first + j (0 behind the last ray).  Trip counts are wave-uniform.
__device__ __forceinline__ uint32_t wave_live_counts(const float *__restrict__ w, int n_rays, int spr, int first, int lane) {
    uint32_t mine = 0;
    for (int j = 0; j < 64; ++j) {
        const int r = first + j;
        if (r >= n_rays) break;
        const float *row = w + (size_t)r * (size_t)spr;
        uint32_t c = 0;
        for (int i0 = 0; i0 < spr; i0 += 64) {
            const int i = i0 + lane;
            const bool live = i < spr && row[i] > 0.0f; // a NaN weight is not live
            c += (uint32_t)__popcll(__ballot(live));
        }
        if (lane == j) mine = c;
    }
    return mine;
}

__global__ __launch_bounds__(kB) void k_normal_block_sums(const float *__restrict__ w, int n_rays, int spr, uint32_t *__restrict__ count,
                                                         uint32_t *__restrict__ bsum) {
    __shared__ uint32_t s[kB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kB + threadIdx.x;
    const uint32_t mine = wave_live_counts(w, n_rays, spr, blockIdx.x * kB + wave * 64, lane);
    if (r < n_rays) count[r] = mine;
    const uint32_t inc = wave_inclusive(mine, lane);
    if (lane == 63) s[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kB / 64; ++k) t += s[k];
        bsum[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kB) void k_normal_scan_sums(uint32_t *__restrict__ bsum, uint32_t n_blocks, uint32_t *__restrict__ totals) {
    __shared__ uint32_t s[kB / 64];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += (uint32_t)kB) { // uniform trip count: every thread reaches the barriers
        const uint32_t i = b0 + threadIdx.x;
        uint32_t v = i < n_blocks ? bsum[i] : 0u, sum;
        block_exclusive(v, sum, s);
        if (i < n_blocks) bsum[i] = v + carry;
        carry += sum;
    }
    if (threadIdx.x == 0) { totals[0] = carry; totals[1] = 0u; }
}

__global__ __launch_bounds__(kB) void k_normal_scan_add(const float *__restrict__ w, int n_rays, int spr, const uint32_t *__restrict__ count,
                                                       const uint32_t *__restrict__ bsum, uint32_t *__restrict__ base,
                                                       uint32_t *__restrict__ list) {
    __shared__ uint32_t s[kB / 64];
    __shared__ uint32_t s_base[kB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kB + threadIdx.x;
    uint32_t v = r < n_rays ? count[r] : 0u, sum;
    block_exclusive(v, sum, s);
    v += bsum[blockIdx.x];
    if (r < n_rays) base[r] = v;
    s_base[threadIdx.x] = v;
    __syncthreads();
    // the same walk as the count: entry (base + rank among the ray's live samples) = the sample's index in the pass
    const int first = blockIdx.x * kB + wave * 64;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j = 0; j < 64; ++j) {
        const int ray = first + j;
        if (ray >= n_rays) break;
        const float *row = w + (size_t)ray * (size_t)spr;
        uint32_t at = s_base[wave * 64 + j];
        for (int i0 = 0; i0 < spr; i0 += 64) {
            const int i = i0 + lane;
            const bool live = i < spr && row[i] > 0.0f;
            const unsigned long long m = __ballot(live);
            if (live) list[at + (uint32_t)__popcll(m & below)] = (uint32_t)ray * (uint32_t)spr + (uint32_t)i;
            at += (uint32_t)__popcll(m);
        }
    }
}

__global__ __launch_bounds__(kB) void k_normal_stencil(NormalStencilArgs a) {
    const uint32_t j = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (j >= a.n_live) return;
    float p[3];
    if (a.list) {
        const uint32_t s = a.list[j];
        const uint32_t ray = s / (uint32_t)a.spr;
        const float t = a.t[s];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float o = a.origins ? a.origins[3 * (size_t)ray + c] : a.origin[c];
            p[c] = __fadd_rn(o, __fmul_rn(a.dirs[3 * (size_t)ray + c], t));
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.src[(size_t)c * a.src_stride + j];
    }
    const size_t L = a.n_live, plane = 6 * L;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int axis = k >> 1;
        const float moved = (k & 1) ? __fsub_rn(p[axis], a.h) : __fadd_rn(p[axis], a.h);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.pts[(size_t)c * plane + (size_t)k * L + j] = c == axis ? moved : p[c]; // contiguous in j across the wave
    }
}

// g of live sample / point j on axis `axis`
__device__ __forceinline__ float central_difference(const float *__restrict__ pts, const float *__restrict__ sigma, size_t L, size_t j, int axis) {
    const size_t plus = (size_t)(2 * axis) * L + j, minus = plus + L;
    const float den = __fsub_rn(pts[(size_t)axis * 6 * L + plus], pts[(size_t)axis * 6 * L + minus]);
    const float num = __fsub_rn(sigma[plus], sigma[minus]);
    return den == 0.0f ? 0.0f : __fdiv_rn(num, den);
}

__global__ __launch_bounds__(kB) void k_normal_reduce(NormalReduceArgs a) {
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= a.n_rays) return;
    const uint32_t n = a.count[r], b = a.base[r];
    float G[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t q = 0; q < n; ++q) {
        const size_t j = (size_t)b + q;
        const float wi = a.w[a.list[j]];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[c] = __fadd_rn(G[c], __fmul_rn(wi, central_difference(a.pts, a.sigma, a.n_live, j, c)));
    }
    // sqrtf, not __fsqrt_rn (the native, approximate square root in this toolchain): sqrtf is correctly rounded under hipcc's default
    // -fhip-fp32-correctly-rounded-divide-sqrt, as in isosurface_kernels.hip
    const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(G[0], G[0]), __fmul_rn(G[1], G[1])), __fmul_rn(G[2], G[2])));
    const bool ok = len > 0.0f && len < __builtin_inff(); // false for 0, inf and NaN
    float *o = a.normals + 3 * (size_t)r;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = ok ? __fdiv_rn(-G[c], len) : 0.0f;
}

__global__ __launch_bounds__(kB) void k_normal_combine(NormalCombineArgs a) {
    const uint32_t j = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (j >= a.n_live) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.grad[(size_t)c * a.dst_stride + j] = central_difference(a.pts, a.sigma, a.n_live, j, c);
}

} // namespace

hipError_t launch_normal_list(const NormalListArgs &a, hipStream_t st) {
    if (a.n_rays <= 0 || a.spr <= 0) return hipErrorInvalidValue;
    if (!a.w || !a.count || !a.base || !a.bsum || !a.totals || !a.list) return hipErrorInvalidValue;
    if ((long long)a.n_rays * a.spr > 0x3fffffffLL) return hipErrorInvalidValue; // sample indices and counts fit 32 bits
    const unsigned n_blocks = ((unsigned)a.n_rays + kB - 1) / kB;
    hipLaunchKernelGGL(k_normal_block_sums, dim3(n_blocks), dim3(kB), 0, st, a.w, a.n_rays, a.spr, a.count, a.bsum);
    hipLaunchKernelGGL(k_normal_scan_sums, dim3(1), dim3(kB), 0, st, a.bsum, n_blocks, a.totals);
    hipLaunchKernelGGL(k_normal_scan_add, dim3(n_blocks), dim3(kB), 0, st, a.w, a.n_rays, a.spr, a.count, a.bsum, a.base, a.list);
    return hipGetLastError();
}

hipError_t launch_normal_stencil(const NormalStencilArgs &a, hipStream_t st) {
    if (a.n_live == 0) return hipSuccess;
    if (!a.pts || (a.list ? (!a.dirs || !a.t || a.spr <= 0) : !a.src)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_normal_stencil, dim3((a.n_live + kB - 1) / kB), dim3(kB), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_normal_reduce(const NormalReduceArgs &a, hipStream_t st) {
    if (a.n_rays <= 0) return hipSuccess;
    if (!a.count || !a.base || !a.list || !a.w || !a.pts || !a.sigma || !a.normals) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_normal_reduce, dim3(((unsigned)a.n_rays + kB - 1) / kB), dim3(kB), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_normal_combine(const NormalCombineArgs &a, hipStream_t st) {
    if (a.n_live == 0) return hipSuccess;
    if (!a.pts || !a.sigma || !a.grad) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_normal_combine, dim3((a.n_live + kB - 1) / kB), dim3(kB), 0, st, a);
    return hipGetLastError();
}
