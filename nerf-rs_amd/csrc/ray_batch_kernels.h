// ray_batch_kernels.h -- launch interface of the ray-batch kernels (nerf_render_rays; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One pass of a ray batch: n_rays caller rays starting at batch ray `first_ray`; every pointer is already offset to the pass.
struct BatchPrepareArgs {
    int n_rays;
    uint32_t first_ray;        // rng_index == NULL: ray r of the pass draws from index first_ray + r
    const float *dirs;         // n_rays x 3, the caller's
    int normalize;             // != 0: Vec3::normalize (k_ray_dirs' arithmetic); 0: copied as they are
    const float *bounds;       // n_rays x 2 {near, far}, or NULL: near_, far_ for every ray
    const uint32_t *rng_index; // n_rays, or NULL
    float near_, far_;
    int count;                 // coarse samples per ray
    uint32_t seed_lo, seed_hi;
    float *dirs_out;           // n_rays x 3: the directions the networks see
    float *t_out;              // n_rays x count: stratified_samples over [near_r, far_r], Philox stream 0 (k_stratified's arithmetic)
    float *far_out;            // n_rays (required with bounds, else unused): far_r, for ResampleArgs / CompositeArgs .far_per_ray
};
hipError_t launch_batch_prepare(const BatchPrepareArgs &a, hipStream_t st);

// (o_r, d_r, t[r][k]) -> the inputs of an MLP_MODE_POINTS launch over the pass's n = n_rays x spr samples: pts_soa (3 planes of n floats,
// fl(o + fl(d t)) per coordinate -- the bits MLP_MODE_RAYS forms) and dirs_aos (n x 3, the ray's direction per sample).
struct BatchPointsArgs {
    int n_rays, spr;
    const float *origins; // n_rays x 3
    const float *dirs;    // n_rays x 3 (BatchPrepareArgs.dirs_out)
    const float *t;       // n_rays x spr
    float *pts_soa;       // 3 x n
    float *dirs_aos;      // n x 3
};
hipError_t launch_batch_points(const BatchPointsArgs &a, hipStream_t st);
