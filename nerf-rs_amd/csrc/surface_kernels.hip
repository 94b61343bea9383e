// surface_kernels.hip -- where a ray meets the surface: the quantile depths of a ray batch and the compaction of the rays that hit into a
// point list.  The contract (every rounding) is in include/nerf_mi355x.h, "quantile depth and point clouds";
// tests/helpers/surface_restatement.py restates it.
//
//   k_ray_quantiles   one ray per lane: walks the ray's compositing weights front to back, cum = fl(cum + w_i), and keeps for each of
//                     up to 8 targets q the position t_i of the first sample with cum >= q
//   k_point_flags     per ray the keep flag (opacity >= min_opacity and a crossing), per 256 rays their number; folds the previous
//                     pass's total into the running offset
//   (the scan of the block sums is launch_clip_scan, ray_clip_kernels.hip: one workgroup, exclusive prefix sums in place, the total)
//   k_point_scatter   per kept ray its rank in the pass -> the pass's list of kept rays
//   k_point_write     one thread per kept ray of the pass: the point record at (running offset + rank)
//   k_point_total     one thread, behind the last pass: the full count
// Every output position is fixed by prefix sums: no atomics, no kernel waits for another workgroup, the same bits in every run; the
// running offset between passes never leaves the device.
// Built like sampling_kernels.hip: IEEE f32 without contraction, correctly rounded divide.  Wave64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.hip.h"
#include "ray_clip_kernels.h"
#include "surface_kernels.h"

namespace {

constexpr int kB = kSurfaceBlock;
static_assert(kB == kScanBlock && kB == kClipBlock, "four waves of 64 rays per workgroup; the scan of the block sums is the clip's");

// ---- quantile depths ------------------------------------------------------------------------------------------------------------------
// cum must be the sequential f32 sum -- its last value is the opacity the compositing kernel wrote, bit for bit -- so a ray is one lane's
// walk and a wave is 64 consecutive rays, as in k_composite.  Global reads stay line-granular the same way: the wave stages kChunk (16)
// samples of w and t of its 64 rays at a time in LDS (16 consecutive floats = one 64-B line per ray and array), rows padded to an odd
// stride so that the per-lane walk is bank-conflict free; all loads are issued before the first LDS store and none is predicated (indices
// are clamped instead; a clamped slot is never read).  One wave per workgroup, 8.5 KiB of LDS.
// Targets and results live in registers (the loops over kSurfaceMaxQuantiles are unrolled); `pending` holds one bit per target not yet
// reached, so a target that is found costs one bit test per sample.  Once no lane of the wave has a pending target the remaining chunks
// are not read.
constexpr int kChunk = 16;
constexpr int kStride = kChunk + 1;

__global__ __launch_bounds__(64) void k_ray_quantiles(RayQuantileArgs a) {
    __shared__ float s_w[64 * kStride], s_t[64 * kStride];
    const int lane = threadIdx.x;
    const int ray0 = blockIdx.x * 64;
    const int n = a.n;
    const int my_ray = ray0 + lane;
    const bool live = my_ray < a.n_rays;
    const int sub = lane & 15, rq = lane >> 4; // staging: 4 rays x 16 samples per wave-instruction
    float cum = 0.0f;
    float res[kSurfaceMaxQuantiles];
#pragma unroll
    for (int j = 0; j < kSurfaceMaxQuantiles; ++j) res[j] = 0.0f;
    unsigned pending = live ? (1u << a.n_q) - 1u : 0u;
    for (int c0 = 0; c0 < n; c0 += kChunk) {
        if (__ballot(pending != 0u) == 0ull) break; // wave-uniform, and the wave is the workgroup: nobody waits at a barrier below
        const int cs = n - c0 < kChunk ? n - c0 : kChunk;
        float vw[16], vt[16];
        const int se = sub < cs ? sub : cs - 1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            int gr = ray0 + 4 * k + rq; gr = gr < a.n_rays ? gr : a.n_rays - 1;
            const size_t at = (size_t)gr * n + c0 + se;
            vw[k] = a.w[at]; vt[k] = a.t[at];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int rr = 4 * k + rq;
            s_w[rr * kStride + se] = vw[k]; s_t[rr * kStride + se] = vt[k]; // clamped duplicates carry the same value to the same slot
        }
        __syncthreads();
        for (int i = 0; i < cs; ++i) {
            cum = __fadd_rn(cum, s_w[lane * kStride + i]);
            if (pending) {
                const float ti = s_t[lane * kStride + i];
#pragma unroll
                for (int j = 0; j < kSurfaceMaxQuantiles; ++j)
                    if ((pending >> j & 1u) && cum >= a.q[j]) { res[j] = ti; pending &= ~(1u << j); } // a NaN sum reaches nothing
            }
        }
        __syncthreads();
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < kSurfaceMaxQuantiles; ++j)
            if (j < a.n_q) a.out[(size_t)j * a.plane_stride + my_ray] = res[j];
    }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------------
// kept: the ray reached the quantile (depth_q is the position of a sample; +-0 = no crossing) and is opaque enough; NaN keeps nothing
__device__ __forceinline__ bool kept(const PointGatherArgs &a, int r) { return r < a.n_rays && a.opacity[r] >= a.min_opacity && a.depth_q[r] != 0.0f; }

__global__ __launch_bounds__(kB) void k_point_flags(PointGatherArgs a) {
    __shared__ uint32_t s[kB / 64];
    const int r = blockIdx.x * kB + threadIdx.x;
    // the launches of a render are ordered on its stream: the previous pass's records are written, its total is not yet overwritten
    if (r == 0) { a.state->running += a.state->total; a.state->total = 0u; }
    const uint32_t c = block_count(kept(a, r), s);
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = c;
}

__global__ __launch_bounds__(kB) void k_point_scatter(PointGatherArgs a) {
    __shared__ uint32_t s[kB / 64];
    const int r = blockIdx.x * kB + threadIdx.x;
    const bool keep = kept(a, r);
    uint32_t rank = keep ? 1u : 0u, sum;
    block_exclusive(rank, sum, s);
    if (keep) a.ray_of[a.bsum[blockIdx.x] + rank] = (uint32_t)r;
}

__global__ __launch_bounds__(kB) void k_point_write(PointGatherArgs a) {
    const uint32_t j = blockIdx.x * (uint32_t)kB + threadIdx.x;
    if (j >= a.state->total) return;
    const uint32_t at = a.state->running + j;
    if (at >= a.capacity) return; // counted, not written
    const size_t r = a.ray_of[j], p = at;
    const float dq = a.depth_q[r], A = a.opacity[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = a.origins ? a.origins[3 * r + c] : a.origin[c];
        a.xyz_out[3 * p + c] = __fadd_rn(o, __fmul_rn(a.dirs[3 * r + c], dq));
        a.rgb_out[3 * p + c] = __fdiv_rn(a.rgb[3 * r + c], A);
    }
    if (a.normals_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normals_out[3 * p + c] = a.normals[3 * r + c];
    }
    if (a.ray_out) a.ray_out[p] = a.first_ray + (uint32_t)r;
    if (a.depth_out) a.depth_out[p] = dq;
    if (a.opacity_out) a.opacity_out[p] = A;
}

__global__ void k_point_total(PointState *state, uint32_t *n_points) {
    const uint32_t n = state->running + state->total;
    state->running = n; state->total = 0u;
    if (n_points) *n_points = n;
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + kB - 1) / kB); }

} // namespace

hipError_t launch_ray_quantiles(const RayQuantileArgs &a, hipStream_t st) {
    if (a.n_rays <= 0) return hipSuccess;
    if (a.n <= 0 || a.n_q < 1 || a.n_q > kSurfaceMaxQuantiles || !a.w || !a.t || !a.out) return hipErrorInvalidValue;
    if ((long long)a.n_rays * a.n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ray_quantiles, dim3(((unsigned)a.n_rays + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_point_gather(const PointGatherArgs &a, hipStream_t st) {
    if (a.n_rays <= 0) return hipSuccess;
    if (!a.dirs || !a.depth_q || !a.rgb || !a.opacity || !a.bsum || !a.ray_of || !a.state || !a.xyz_out || !a.rgb_out ||
        (a.normals_out && !a.normals))
        return hipErrorInvalidValue;
    const dim3 grid(blocks_of(a.n_rays)), block(kB);
    hipLaunchKernelGGL(k_point_flags, grid, block, 0, st, a);
    const hipError_t e = launch_clip_scan(a.bsum, a.n_rays, &a.state->total, st); // writes state->total and clears state->unused
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_point_scatter, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_point_write, grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_point_total(PointState *state, uint32_t *n_points, hipStream_t st) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_point_total, dim3(1), dim3(1), 0, st, state, n_points);
    return hipGetLastError();
}
