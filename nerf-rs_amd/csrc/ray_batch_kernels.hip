// ray_batch_kernels.hip -- what a caller-supplied ray batch (nerf_render_rays) needs in front of the networks.
//
//   k_batch_prepare   the caller's directions -> unit directions (Vec3::normalize, k_ray_dirs' arithmetic) and the coarse samples
//                     (stratified_samples over the ray's own [near, far], k_stratified's arithmetic, Philox stream 0 of the ray's index)
//   k_batch_points    per-ray origins: the points and per-sample directions of an MLP_MODE_POINTS launch
// Built like sampling_kernels.hip: IEEE f32 without contraction, correctly rounded divide and sqrt -- a batch made of a camera's rays
// carries the bits of the image render.  Both kernels are streaming bookkeeping (wave64, 256-thread workgroups, no LDS, no scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.hip.h"
#include "ray_batch_kernels.h"

// one thread per (ray, group of 4 samples), as k_stratified; the thread of group 0 also writes the ray's direction and far
__global__ __launch_bounds__(256) void k_batch_prepare(BatchPrepareArgs a) {
    const int quads = (a.count + 3) >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)a.n_rays * quads) return;
    const int r = (int)(gid / quads), q = (int)(gid % quads);
    const float near_ = a.bounds ? a.bounds[2 * (size_t)r] : a.near_, far_ = a.bounds ? a.bounds[2 * (size_t)r + 1] : a.far_;
    if (q == 0) {
        const float dx = a.dirs[3 * (size_t)r], dy = a.dirs[3 * (size_t)r + 1], dz = a.dirs[3 * (size_t)r + 2];
        float *o = a.dirs_out + 3 * (size_t)r;
        if (a.normalize) {
            const float len = sqrtf(dx * dx + dy * dy + dz * dz);
            o[0] = dx / len; o[1] = dy / len; o[2] = dz / len;
        } else {
            o[0] = dx; o[1] = dy; o[2] = dz;
        }
        if (a.bounds) a.far_out[r] = far_;
    }
    const uint32_t idx = a.rng_index ? a.rng_index[r] : a.first_ray + (uint32_t)r;
    uint32_t rnd[4];
    philox4x32(a.seed_lo, a.seed_hi, idx, 0u, (uint32_t)q, 0u, rnd);
    const float interval = (far_ - near_) / (float)a.count;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * q + e;
        if (k < a.count) {
            const float lower = near_ + (float)k * interval;
            const float upper = lower + interval;
            a.t_out[(size_t)r * a.count + k] = lower + (upper - lower) * u01(rnd[e]);
        }
    }
}

// One thread per output float of each array, so that both stores are contiguous across a wave: float i of dirs_aos is component i % 3 of
// sample i / 3, float i of pts_soa is sample i % n of plane i / n.  3 n <= 0xBFFFFFFD (n <= 0x3fffffff per pass): the index is 64-bit.
__global__ __launch_bounds__(256) void k_batch_points(BatchPointsArgs a) {
    const size_t n = (size_t)a.n_rays * (size_t)a.spr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * n) return;
    {
        const size_t sample = i / 3;
        const int c = (int)(i - 3 * sample);
        a.dirs_aos[i] = a.dirs[3 * (sample / (size_t)a.spr) + c];
    }
    const int c = (int)(i / n);
    const size_t sample = i - (size_t)c * n;
    const size_t ray = sample / (size_t)a.spr;
    a.pts_soa[i] = __fadd_rn(a.origins[3 * ray + c], __fmul_rn(a.dirs[3 * ray + c], a.t[sample]));
}

hipError_t launch_batch_prepare(const BatchPrepareArgs &a, hipStream_t st) {
    if (a.n_rays <= 0 || a.count <= 0) return hipSuccess;
    if (!a.dirs || !a.dirs_out || !a.t_out || (a.bounds && !a.far_out)) return hipErrorInvalidValue;
    const long long total = (long long)a.n_rays * ((a.count + 3) / 4);
    hipLaunchKernelGGL(k_batch_prepare, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_points(const BatchPointsArgs &a, hipStream_t st) {
    if (a.n_rays <= 0 || a.spr <= 0) return hipSuccess;
    if (!a.origins || !a.dirs || !a.t || !a.pts_soa || !a.dirs_aos) return hipErrorInvalidValue;
    const size_t total = 3 * (size_t)a.n_rays * (size_t)a.spr;
    if (total > (size_t)3 * 0x3fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_batch_points, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
