// ray_clip_kernels.hip -- an occupancy grid in front of a ray batch (include/nerf_mi355x.h, "ray clipping").
//
//   k_occupancy_dilate  one thread per output word: a cell is set iff an input cell within Chebyshev distance r is
//   k_clip_rays         one lane per ray: slab test + cell walk (ray_clip_core.h, the function nerf_debug_clip_rays calls on the host);
//                       optionally the hits per workgroup and the outputs of the missed rays of a clipped render
//   k_clip_scan         ONE workgroup: exclusive prefix sums of the workgroups' hit counts, the total
//   k_clip_gather       hit ray r -> compacted ray j (ascending r): directions, origins, clipped bounds, rng index
//   k_clip_scatter      compacted outputs j -> ray r
// The occupancy words are read from global memory (128^3 cells = 256 KiB: resident in L2, too large for LDS).  Every output position is
// fixed by prefix sums: no atomics, no kernel waits for another workgroup, the same bits in every run.
// Built like ray_batch_kernels.hip: IEEE f32 without contraction, correctly rounded divide and sqrt.  Wave64, 256-thread workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.hip.h"
#include "ray_clip_core.h"
#include "ray_clip_kernels.h"

namespace {

constexpr int kB = kClipBlock;
static_assert(kB == kScanBlock, "four waves of 64 rays per workgroup (block_scan.hip.h)");

// any set bit among the linear cells c0 .. c1 (inclusive; both inside the grid)
__device__ __forceinline__ bool any_set(const uint32_t *__restrict__ bits, int c0, int c1) {
    const int w0 = c0 >> 5, w1 = c1 >> 5;
    for (int w = w0; w <= w1; ++w) {
        uint32_t mask = 0xffffffffu;
        if (w == w0) mask &= 0xffffffffu << (c0 & 31);
        if (w == w1) mask &= 0xffffffffu >> (31 - (c1 & 31));
        if (bits[w] & mask) return true;
    }
    return false;
}

// Works on cells, not on words: a row of nx cells may start anywhere in a word.
__global__ __launch_bounds__(kB) void k_occupancy_dilate(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int nx, int ny, int nz, int r,
                                                        int n_cells, int n_words) {
    const int w = blockIdx.x * kB + threadIdx.x;
    if (w >= n_words) return;
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const long long cell = 32ll * w + b;
        if (cell >= n_cells) break;
        const int c = (int)cell, ix = c % nx, iy = (c / nx) % ny, iz = c / (nx * ny);
        const int x0 = max(ix - r, 0), x1 = min(ix + r, nx - 1);
        bool set = false;
        for (int z = max(iz - r, 0); z <= min(iz + r, nz - 1) && !set; ++z)
            for (int y = max(iy - r, 0); y <= min(iy + r, ny - 1) && !set; ++y) {
                const int row = nx * (y + ny * z);
                set = any_set(in, row + x0, row + x1);
            }
        if (set) word |= 1u << b;
    }
    out[w] = word;
}

__global__ __launch_bounds__(kB) void k_clip_rays(ClipRaysArgs a) {
    __shared__ uint32_t s[kB / 64];
    const int r = blockIdx.x * kB + threadIdx.x;
    bool hit = false;
    if (r < a.n_rays) {
        float near_r, far_r;
        const nerfclip::Result res = nerfclip::clip_batch_ray(a.bits, a.lo, a.step, a.dims, a.origins, a.per_ray_origins, a.dirs, a.normalize,
                                                              a.near_, a.far_, a.bounds, (size_t)r, &near_r, &far_r);
        hit = res.hit != 0;
        a.bounds_out[2 * (size_t)r] = res.t_first;
        a.bounds_out[2 * (size_t)r + 1] = res.t_last;
        a.hit_out[r] = hit ? 1 : 0;
        if (!hit) {
            if (a.rgb_fill) { float *o = a.rgb_fill + 3 * (size_t)r; o[0] = a.bg[0]; o[1] = a.bg[1]; o[2] = a.bg[2]; }
            if (a.depth_fill) a.depth_fill[r] = 0.0f;
            if (a.opacity_fill) a.opacity_fill[r] = 0.0f;
        }
    }
    if (a.bsum) { // uniform: every thread of the workgroup reaches the barrier
        const uint32_t c = block_count(hit, s);
        if (threadIdx.x == 0) a.bsum[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(kB) void k_clip_scan(uint32_t *__restrict__ bsum, uint32_t n_blocks, uint32_t *__restrict__ totals) {
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

__global__ __launch_bounds__(kB) void k_clip_gather(ClipGatherArgs a) {
    __shared__ uint32_t s[kB / 64];
    const int r = blockIdx.x * kB + threadIdx.x;
    const bool hit = r < a.n_rays && a.hit[r] != 0;
    uint32_t v = hit ? 1u : 0u, sum;
    block_exclusive(v, sum, s);
    if (!hit) return;
    const size_t j = (size_t)a.bsum[blockIdx.x] + v, q = (size_t)r;
    a.ray_of[j] = (uint32_t)r;
#pragma unroll
    for (int c = 0; c < 3; ++c) a.dirs_c[3 * j + c] = a.dirs[3 * q + c];
    if (a.origins) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.origins_c[3 * j + c] = a.origins[3 * q + c];
    }
    a.bounds_c[2 * j] = a.clip_bounds[2 * q];
    a.bounds_c[2 * j + 1] = a.clip_bounds[2 * q + 1];
    a.rng_c[j] = a.rng_index ? a.rng_index[q] : (uint32_t)r;
}

__global__ __launch_bounds__(kB) void k_clip_scatter(ClipScatterArgs a) {
    const uint32_t j = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (j >= a.n_hit) return;
    const size_t r = a.ray_of[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb[3 * r + c] = a.rgb_c[3 * (size_t)j + c];
    if (a.depth) a.depth[r] = a.depth_c[j];
    if (a.opacity) a.opacity[r] = a.opacity_c[j];
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kB - 1) / kB); }

} // namespace

hipError_t launch_occupancy_dilate(const uint32_t *in, uint32_t *out, int nx, int ny, int nz, int radius, hipStream_t st) {
    if (!in || !out || nx < 1 || ny < 1 || nz < 1 || radius < 1) return hipErrorInvalidValue;
    const long long n = (long long)nx * ny * nz;
    if (n > 0x7fffffffLL) return hipErrorInvalidValue;
    const int n_words = (int)((n + 31) / 32);
    hipLaunchKernelGGL(k_occupancy_dilate, dim3(blocks_of(n_words)), dim3(kB), 0, st, in, out, nx, ny, nz, radius, (int)n, n_words);
    return hipGetLastError();
}

hipError_t launch_clip_rays(const ClipRaysArgs &a, hipStream_t st) {
    if (a.n_rays <= 0) return hipSuccess;
    if (!a.bits || !a.origins || !a.dirs || !a.bounds_out || !a.hit_out) return hipErrorInvalidValue;
    for (int k = 0; k < 3; ++k)
        if (a.dims[k] < 1) return hipErrorInvalidValue;
    if ((long long)a.dims[0] * a.dims[1] > 0x7fffffffLL || (long long)a.dims[0] * a.dims[1] * a.dims[2] > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clip_rays, dim3(blocks_of(a.n_rays)), dim3(kB), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_clip_scan(uint32_t *bsum, int n_rays, uint32_t *totals, hipStream_t st) {
    if (n_rays <= 0 || !bsum || !totals) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clip_scan, dim3(1), dim3(kB), 0, st, bsum, blocks_of(n_rays), totals);
    return hipGetLastError();
}

hipError_t launch_clip_gather(const ClipGatherArgs &a, hipStream_t st) {
    if (a.n_rays <= 0) return hipSuccess;
    if (!a.hit || !a.bsum || !a.dirs || !a.clip_bounds || !a.ray_of || !a.dirs_c || !a.bounds_c || !a.rng_c || (a.origins && !a.origins_c))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clip_gather, dim3(blocks_of(a.n_rays)), dim3(kB), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_clip_scatter(const ClipScatterArgs &a, hipStream_t st) {
    if (a.n_hit == 0) return hipSuccess;
    if (!a.ray_of || !a.rgb_c || !a.rgb || (a.depth && !a.depth_c) || (a.opacity && !a.opacity_c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_clip_scatter, dim3(blocks_of(a.n_hit)), dim3(kB), 0, st, a);
    return hipGetLastError();
}
