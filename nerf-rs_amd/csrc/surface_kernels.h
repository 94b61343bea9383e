// surface_kernels.h -- launch interface of the quantile-depth walk and of the point-cloud compaction (nerf_render_rays_quantiles,
// nerf_render_rays_points, nerf_stage_ray_quantiles, nerf_stage_gather_points; internal).  The contract is in include/nerf_mi355x.h
// ("quantile depth and point clouds").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kSurfaceBlock = 256;    // threads per workgroup of the compaction kernels = rays per scan block (ray_clip_kernels.h kClipBlock)
constexpr int kSurfaceMaxQuantiles = 8; // NERF_MAX_QUANTILES

// Per ray the positions at which the running sum of its weights first reaches each of n_q targets.
struct RayQuantileArgs {
    int n_rays, n;       // rays, samples per ray
    const float *w;      // n_rays x n: the compositing weights (CompositeArgs.w_out)
    const float *t;      // n_rays x n: the samples' positions
    int n_q;             // 1 .. kSurfaceMaxQuantiles
    float q[kSurfaceMaxQuantiles];
    float *out;          // plane k (of n_q) starts at out + k * plane_stride; n_rays floats each
    size_t plane_stride;
};
hipError_t launch_ray_quantiles(const RayQuantileArgs &a, hipStream_t st);

// The words the compaction keeps on the device between the passes of a render.
struct PointState {
    uint32_t total;   // kept rays of the pass under way (the scan's total) ...
    uint32_t unused;  // ... and the word the scan clears behind it
    uint32_t running; // kept rays of the passes before it
    uint32_t pad;
};

// One pass of the compaction: rays [0, n_rays) of the pass are rays first_ray + r of the batch; every per-ray input pointer is the pass's.
struct PointGatherArgs {
    int n_rays;
    uint32_t first_ray;
    const float *origins;  // n_rays x 3, or NULL: `origin` for every ray
    float origin[3];
    const float *dirs;     // n_rays x 3: the directions the networks saw
    const float *depth_q;  // n_rays
    const float *rgb;      // n_rays x 3: C, the colour over a black background
    const float *opacity;  // n_rays
    const float *normals;  // n_rays x 3, or NULL
    float min_opacity;
    uint32_t capacity;     // points the outputs hold: a point whose position is not below it is counted, not written
    // workspace
    uint32_t *bsum;        // ceil(n_rays / 256)
    uint32_t *ray_of;      // n_rays: the kept rays of the pass (pass-local index), ascending
    PointState *state;     // cleared before the first pass
    // outputs, the whole batch's: position = state->running + rank of the ray among the kept rays of the pass
    float *xyz_out, *rgb_out, *normals_out; // x 3; normals_out NULL without normals
    uint32_t *ray_out;                      // optional
    float *depth_out, *opacity_out;         // optional
};
// flags + block sums, the scan (ray_clip_kernels.h launch_clip_scan), the scatter of the kept rays, the records: four launches
hipError_t launch_point_gather(const PointGatherArgs &a, hipStream_t st);
// behind the last pass: *n_points (device, optional) = the full count; state->running holds it afterwards and state->total is 0
hipError_t launch_point_total(PointState *state, uint32_t *n_points, hipStream_t st);
