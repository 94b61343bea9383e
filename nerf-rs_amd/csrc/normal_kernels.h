// normal_kernels.h -- launch interface of the density-gradient / ray-normal kernels (nerf_density_gradient_batch,
// nerf_render_rays_normals; internal).  The contract is in include/nerf_mi355x.h ("surface normals").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kNormalBlock = 256; // threads per workgroup of every kernel here = rays per scan block

// Per pass of a ray batch: which samples are live (weight > 0), where each ray's live samples start in the compacted list.
struct NormalListArgs {
    const float *w;      // n_rays x spr: the compositing weights (CompositeArgs.w_out)
    int n_rays, spr;
    uint32_t *count;     // n_rays: live samples of the ray
    uint32_t *base;      // n_rays: exclusive prefix sum of count over the pass
    uint32_t *bsum;      // ceil(n_rays / 256): block sums, then their exclusive prefix sums in place
    uint32_t *totals;    // 2 words: {live samples of the pass, 0} -- the 8 bytes the host reads
    uint32_t *list;      // capacity n_rays x spr: sample index (ray * spr + k) of every live sample, rays ascending, k ascending
};
// three launches (block sums, one-workgroup scan, scan-add + list); the host then reads totals
hipError_t launch_normal_list(const NormalListArgs &a, hipStream_t st);

// The six stencil points of each of n_live samples into pts (3 planes of 6 n_live floats, the layout of an MLP_MODE_POINTS launch):
// slot k * n_live + j, k = 2 * axis + (0: plus, 1: minus), holds sample j with coordinate `axis` replaced by fl(p_axis + h) / fl(p_axis - h).
// Ray form (list != NULL): sample j is list[j] = ray * spr + k at fl(o + fl(d * t)); o = origins[ray], or `origin` when origins is NULL.
// Point form (list == NULL): sample j is the caller's point j (planes `src_stride` floats apart).
struct NormalStencilArgs {
    uint32_t n_live;
    float h;
    const uint32_t *list;
    int spr;
    const float *origins; // n_rays x 3 or NULL
    float origin[3];
    const float *dirs;    // n_rays x 3
    const float *t;       // n_rays x spr
    const float *src;     // point form: 3 planes
    size_t src_stride;
    float *pts;           // 3 x 6 n_live
};
hipError_t launch_normal_stencil(const NormalStencilArgs &a, hipStream_t st);

// One thread per ray: G = sum over the ray's live samples, in order, of w * g; n = -G / |G| (zero when |G| is 0 or not finite).
// g per axis = (sigma+ - sigma-) / (p+ - p-), 0 when the denominator is 0; every operation rounded once.
struct NormalReduceArgs {
    int n_rays;
    uint32_t n_live;
    const uint32_t *count, *base, *list;
    const float *w;       // n_rays x spr
    const float *pts;     // 3 x 6 n_live (the stencil)
    const float *sigma;   // 6 n_live
    float *normals;       // n_rays x 3
};
hipError_t launch_normal_reduce(const NormalReduceArgs &a, hipStream_t st);

// Point form: g of each of n_live points, unweighted, into 3 planes `dst_stride` floats apart.
struct NormalCombineArgs {
    uint32_t n_live;
    const float *pts, *sigma;
    float *grad;
    size_t dst_stride;
};
hipError_t launch_normal_combine(const NormalCombineArgs &a, hipStream_t st);
