// ray_clip_kernels.h -- launch interface of the occupancy-grid kernels around a ray batch (nerf_occupancy_dilate, nerf_clip_rays,
// nerf_render_rays_clipped; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kClipBlock = 256; // rays per workgroup of every per-ray kernel here: the unit of the block sums

// out = the cells within Chebyshev distance `radius` of a set cell of `in` (both ceil(N / 32) words, x fastest; the bits behind cell N - 1
// of out are 0).  in and out must not overlap.
hipError_t launch_occupancy_dilate(const uint32_t *in, uint32_t *out, int nx, int ny, int nz, int radius, hipStream_t st);

// One lane per ray: ray_clip_core.h's clip_batch_ray.  Optional extras of the same launch:
//   bsum     per workgroup of kClipBlock rays the number of hits (for the prefix sums below)
//   rgb_fill / depth_fill / opacity_fill   what a MISSED ray of nerf_render_rays_clipped carries: bg, 0, 0 (hit rays are left alone)
struct ClipRaysArgs {
    const uint32_t *bits;
    float lo[3], step[3];
    int32_t dims[3];
    const float *origins;  // n_rays x 3, or 3 floats when per_ray_origins == 0
    int per_ray_origins;
    const float *dirs;     // n_rays x 3
    int n_rays, normalize;
    float near_, far_;
    const float *bounds;   // n_rays x 2 or NULL
    float *bounds_out;     // n_rays x 2
    uint8_t *hit_out;      // n_rays
    uint32_t *bsum;        // ceil(n_rays / kClipBlock) or NULL
    float *rgb_fill, *depth_fill, *opacity_fill; // n_rays x 3, n_rays, n_rays; each may be NULL
    float bg[3];
};
hipError_t launch_clip_rays(const ClipRaysArgs &a, hipStream_t st);

// ONE workgroup: exclusive prefix sums of the block sums in place; totals[0] = the number of hits, totals[1] = 0
hipError_t launch_clip_scan(uint32_t *bsum, int n_rays, uint32_t *totals, hipStream_t st);

// The hit rays in ascending ray order: hit ray r becomes ray j = bsum[r / kClipBlock] + (hits before r in its block) of the compacted batch.
struct ClipGatherArgs {
    int n_rays;
    const uint8_t *hit;
    const uint32_t *bsum;      // scanned
    const float *dirs, *origins /* NULL: shared origin */, *clip_bounds;
    const uint32_t *rng_index; // NULL: ray r draws from index r
    uint32_t *ray_of;          // j -> r
    float *dirs_c, *origins_c, *bounds_c;
    uint32_t *rng_c;
};
hipError_t launch_clip_gather(const ClipGatherArgs &a, hipStream_t st);

// outputs of compacted ray j -> ray ray_of[j]
struct ClipScatterArgs {
    uint32_t n_hit;
    const uint32_t *ray_of;
    const float *rgb_c, *depth_c, *opacity_c;
    float *rgb, *depth, *opacity; // depth / opacity (and their sources) may be NULL
};
hipError_t launch_clip_scatter(const ClipScatterArgs &a, hipStream_t st);
