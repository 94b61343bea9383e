// nerf_queries.cpp -- the device entry points that are not renders (include/nerf_mi355x.h): network evaluation at caller points, density
// batches and grids, occupancy dilation and ray clipping, isosurface meshes and lattice components, density gradients, and the nerf_stage_* calls that run one kernel of the
// render pipeline on caller data.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "components_kernels.h"
#include "isosurface_kernels.h"
#include "mlp_kernel.h"
#include "normal_kernels.h"
#include "ray_clip_core.h"
#include "ray_clip_kernels.h"
#include "sampling_kernels.h"
#include "surface_kernels.h"

#include "nerf_internal.h"

using namespace nerfint;

constexpr size_t F = sizeof(float);

extern "C" {

static int forward_device(nerf_ctx *c, int which, int dtype, const float *d_pts, const float *d_dirs, size_t n, float *d_rgb,
                          float *d_sigma, void *stream) {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (n == 0) return NERF_OK; // src/network.rs:199-201
    if (!d_pts || !d_dirs || !d_rgb || !d_sigma) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    // the kernels index points in int32 and look one persistent-grid stride of tiles ahead (load_raw): keep that in range too
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    DeviceGuard dg(c->device);
    MlpArgs a{};
    a.mode = MLP_MODE_POINTS;
    if (!valid_dtype(dtype)) return fail(c, NERF_ERR_INVALID, "mlp_dtype must be NERF_MLP_F32, NERF_MLP_BF16, NERF_MLP_BF16X3 or NERF_MLP_F16X2");
    if (!available(c->net[which], dtype)) return fail(c, NERF_ERR_STATE, "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range");
    fill_net(c, c->net[which], dtype, a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.dirs_aos = d_dirs; a.sigma_out = d_sigma; a.rgb_out = d_rgb;
    HIP_TRY(c, launch_mlp(c, dtype, a, true, (hipStream_t)stream));
    return NERF_OK;
}

int nerf_forward_batch_device(nerf_ctx *c, int which, const float *d_pts, const float *d_dirs, size_t n, float *d_rgb,
                              float *d_sigma, void *stream) try {
    return forward_device(c, which, NERF_MLP_F32, d_pts, d_dirs, n, d_rgb, d_sigma, stream);
} NERF_CATCH(c)

int nerf_forward_batch(nerf_ctx *c, int which, const float *pts, const float *dirs, size_t n, float *rgb, float *sigma) try {
    return nerf_forward_batch_ex(c, which, NERF_MLP_F32, pts, dirs, n, rgb, sigma);
} NERF_CATCH(c)

int nerf_forward_batch_ex(nerf_ctx *c, int which, int dtype, const float *pts, const float *dirs, size_t n, float *rgb, float *sigma) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (!pts || !dirs || !rgb || !sigma) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    DeviceGuard dg(c->device);
    int rc;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_pts = s.add(F, 3 * n, pts), i_dirs = s.add(F, 3 * n, dirs), i_rgb = s.add(F, 3 * n, nullptr, rgb), i_sig = s.add(F, n, nullptr, sigma);
    if ((rc = s.begin())) return rc;
    unsigned int *d_bad = c->dev<unsigned int>(BUF_NONFINITE);
    const bool watch = split_dtype(dtype) && d_bad;
    if (watch) HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned int), c->stream));
    if ((rc = forward_device(c, which, dtype, s.at(i_pts), s.at(i_dirs), n, s.at(i_rgb), s.at(i_sig), c->stream))) return rc;
    unsigned int bad = 0;
    if (watch) HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    if ((rc = s.finish())) return rc;
    if (bad) {
        char msg[320];
        snprintf(msg, sizeof msg, "%u of %zu points: an operand left the range of the split arithmetic (NERF_MLP_F16X2: |activation| <= 65504) or a "
                 "density was not finite; the outputs are not usable -- use NERF_MLP_BF16X3 or NERF_MLP_F32", bad, n);
        return fail(c, NERF_ERR_STATE, msg);
    }
    return NERF_OK;
} NERF_CATCH(c)

// ---- density queries (f32 sigma-only kernel: MLP_MODE_POINTS without directions, MLP_MODE_GRID) -----------------------------------
// Argument checks come before anything that needs the context or the device, so that a host without a GPU gets the same answers.
// what nerf_density_batch* refuses, in its order; n == 0 passes here and makes the caller return at once
static int density_batch_check(nerf_ctx *c, int which, const void *pts, const void *sigma, size_t n) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (!pts || !sigma) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    return NERF_OK;
}

static int density_batch_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float *d_sigma, hipStream_t st) {
    int rc;
    if ((rc = density_batch_check(c, which, d_pts, d_sigma, n)) || n == 0) return rc;
    DeviceGuard dg(c->device);
    HIP_TRY(c, launch_sigma_points(c, c->net[which], d_pts, n, d_sigma, st));
    return NERF_OK;
}

int nerf_density_batch_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float *d_sigma, void *stream) try {
    return density_batch_device(c, which, d_pts, n, d_sigma, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_density_batch(nerf_ctx *c, int which, const float *pts, size_t n, float *sigma) try {
    int rc;
    if ((rc = density_batch_check(c, which, pts, sigma, n)) || n == 0) return rc;
    DeviceGuard dg(c->device);
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_pts = s.add(F, 3 * n, pts), i_sig = s.add(F, n, nullptr, sigma);
    if ((rc = s.begin())) return rc;
    if ((rc = density_batch_device(c, which, s.at(i_pts), n, s.at(i_sig), c->stream))) return rc;
    return s.finish();
} NERF_CATCH(c)

// everything nerf_density_grid* can refuse without a device; *n_cells = dims[0] dims[1] dims[2]
static int density_grid_check(nerf_ctx *c, int which, const float *lo, const float *step, const int32_t *dims, const void *sigma_out,
                              float threshold, const void *occ_bits, const void *n_occupied, const void *bounds, size_t *n_cells) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!lo || !step || !dims) return fail(c, NERF_ERR_INVALID, "lo, step and dims must not be NULL");
    for (int k = 0; k < 3; ++k) {
        if (dims[k] <= 0) return fail(c, NERF_ERR_INVALID, "dims must be positive");
        if (!std::isfinite(lo[k]) || !std::isfinite(step[k])) return fail(c, NERF_ERR_INVALID, "lo and step must be finite");
    }
    if (!sigma_out && !occ_bits) return fail(c, NERF_ERR_INVALID, "at least one of sigma_out and occ_bits must be given");
    if (occ_bits && !(threshold >= 0.0f)) return fail(c, NERF_ERR_INVALID, "threshold must be >= 0 (and not NaN) when occ_bits is given");
    if (!occ_bits && (n_occupied || bounds)) return fail(c, NERF_ERR_INVALID, "n_occupied and bounds need occ_bits");
    // one launch, no slabs: N within the largest batch (the tighter, device-dependent limit follows once the context is known)
    const size_t limit = c ? max_batch_points(c->n_cus) : max_batch_points(0);
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane > limit || plane * (unsigned long long)dims[2] > limit)
        return fail(c, NERF_ERR_INVALID, "grid too large: dims[0] * dims[1] * dims[2] must fit in one launch (as nerf_forward_batch's n)");
    *n_cells = (size_t)(plane * (unsigned long long)dims[2]);
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    return NERF_OK;
}

// the MLP launch in grid mode and, with d_stats (8 ints, device), the statistics of its occupancy words; arguments already checked
static int density_grid_launch(nerf_ctx *c, int which, const float *lo, const float *step, const int32_t *dims, size_t n_cells,
                               float *d_sigma, float threshold, uint32_t *d_bits, int *d_stats, hipStream_t st) {
    MlpArgs a{};
    a.mode = MLP_MODE_GRID;
    fill_net(c, c->net[which], NERF_MLP_F32, a);
    a.n_points = (int)n_cells; a.sigma_out = d_sigma;
    for (int k = 0; k < 3; ++k) { a.grid_lo[k] = lo[k]; a.grid_step[k] = step[k]; a.grid_n[k] = dims[k]; }
    a.occ_threshold = threshold; a.occ_bits = d_bits;
    HIP_TRY(c, launch_mlp(c, NERF_MLP_F32, a, false, st));
    if (d_stats) HIP_TRY(c, launch_occupancy_stats(d_bits, n_cells, dims[0], dims[1], dims[2], d_stats, st));
    return NERF_OK;
}

static void density_grid_stats_out(const int *h, uint64_t *n_occupied, int32_t *bounds) {
    if (n_occupied) *n_occupied = (uint64_t)(uint32_t)h[0] | ((uint64_t)(uint32_t)h[1] << 32);
    if (bounds) for (int k = 0; k < 6; ++k) bounds[k] = h[2 + k];
}

int nerf_density_grid_device(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float *d_sigma_out,
                             float threshold, uint32_t *d_occ_bits, uint64_t *n_occupied, int32_t bounds[6], void *stream) try {
    size_t n_cells = 0;
    int rc;
    if ((rc = density_grid_check(c, which, lo, step, dims, d_sigma_out, threshold, d_occ_bits, n_occupied, bounds, &n_cells))) return rc;
    DeviceGuard dg(c->device);
    const bool stats = n_occupied || bounds;
    int h[8];
    Staging s(c, BUF_SCRATCH, (hipStream_t)stream);
    const int i_stats = s.opt(stats, sizeof(int), 8, nullptr, h);
    if ((rc = s.begin())) return rc;
    if ((rc = density_grid_launch(c, which, lo, step, dims, n_cells, d_sigma_out, threshold, d_occ_bits, s.at<int>(i_stats), s.st))) return rc;
    if (stats) {
        if ((rc = s.finish())) return rc;
        density_grid_stats_out(h, n_occupied, bounds);
    }
    return NERF_OK;
} NERF_CATCH(c)

int nerf_density_grid(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float *sigma_out,
                      float threshold, uint32_t *occ_bits, uint64_t *n_occupied, int32_t bounds[6]) try {
    size_t n_cells = 0;
    int rc;
    if ((rc = density_grid_check(c, which, lo, step, dims, sigma_out, threshold, occ_bits, n_occupied, bounds, &n_cells))) return rc;
    DeviceGuard dg(c->device);
    // staging: [8 ints of statistics][occupancy words][sigma], each only if asked for
    const bool stats = n_occupied || bounds;
    int h[8];
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_stats = s.opt(stats, sizeof(int), 8, nullptr, h), i_bits = s.opt(occ_bits, sizeof(uint32_t), (n_cells + 31) / 32, nullptr, occ_bits),
              i_sigma = s.opt(sigma_out, F, n_cells, nullptr, sigma_out);
    if ((rc = s.begin())) return rc;
    if ((rc = density_grid_launch(c, which, lo, step, dims, n_cells, s.at(i_sigma), threshold, s.at<uint32_t>(i_bits), s.at<int>(i_stats), c->stream))) return rc;
    if ((rc = s.finish())) return rc;
    if (stats) density_grid_stats_out(h, n_occupied, bounds);
    return NERF_OK;
} NERF_CATCH(c)

// ---- ray clipping (ray_clip_kernels.hip): occupancy dilation and the per-ray span of the occupied cells -----------------------------------
// everything nerf_occupancy_dilate* can refuse without a device; *n_cells = dims[0] dims[1] dims[2]
static int dilate_check(nerf_ctx *c, const uint32_t *in, const int32_t *dims, int radius, const uint32_t *out, size_t *n_cells) {
    if (!in || !dims || !out) return fail(c, NERF_ERR_INVALID, "occ_bits, dims and occ_out must not be NULL");
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 1) return fail(c, NERF_ERR_INVALID, "dims must be positive");
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane > 0x7fffffffull || plane * (unsigned long long)dims[2] > 0x7fffffffull)
        return fail(c, NERF_ERR_INVALID, "grid too large: dims[0] * dims[1] * dims[2] must be at most INT32_MAX");
    *n_cells = (size_t)(plane * (unsigned long long)dims[2]);
    if (radius < 1 || radius > 4) return fail(c, NERF_ERR_INVALID, "radius must be 1, 2, 3 or 4");
    const size_t n_words = (*n_cells + 31) / 32;
    if (in < out + n_words && out < in + n_words) return fail(c, NERF_ERR_INVALID, "occ_bits and occ_out must not overlap");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    return NERF_OK;
}

// the dilation and, when asked for, the statistics of its output (d_stats: 8 ints on the device); arguments already checked
static int dilate_device(nerf_ctx *c, const uint32_t *d_in, const int32_t *dims, int radius, uint32_t *d_out, size_t n_cells, int *d_stats,
                         uint64_t *n_occupied, int32_t *bounds, hipStream_t st) {
    HIP_TRY(c, launch_occupancy_dilate(d_in, d_out, dims[0], dims[1], dims[2], radius, st));
    if (!d_stats) return NERF_OK;
    HIP_TRY(c, launch_occupancy_stats(d_out, n_cells, dims[0], dims[1], dims[2], d_stats, st));
    int h[8];
    HIP_TRY(c, hipMemcpyAsync(h, d_stats, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    density_grid_stats_out(h, n_occupied, bounds);
    return NERF_OK;
}

int nerf_occupancy_dilate_device(nerf_ctx *c, const uint32_t *d_occ_bits, const int32_t dims[3], int radius, uint32_t *d_occ_out,
                                 uint64_t *n_occupied, int32_t bounds[6], void *stream) try {
    size_t n_cells = 0;
    int rc;
    if ((rc = dilate_check(c, d_occ_bits, dims, radius, d_occ_out, &n_cells))) return rc;
    DeviceGuard dg(c->device);
    const bool stats = n_occupied || bounds;
    if (stats && (rc = c->buf[BUF_SCRATCH].ensure(c, 8 * sizeof(int)))) return rc;
    return dilate_device(c, d_occ_bits, dims, radius, d_occ_out, n_cells, stats ? c->dev<int>(BUF_SCRATCH) : nullptr, n_occupied, bounds, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_occupancy_dilate(nerf_ctx *c, const uint32_t *occ_bits, const int32_t dims[3], int radius, uint32_t *occ_out, uint64_t *n_occupied,
                          int32_t bounds[6]) try {
    size_t n_cells = 0;
    int rc;
    if ((rc = dilate_check(c, occ_bits, dims, radius, occ_out, &n_cells))) return rc;
    DeviceGuard dg(c->device);
    // staging: [8 ints of statistics][input words][output words]
    const size_t n_words = (n_cells + 31) / 32;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_stats = s.opt(n_occupied || bounds, sizeof(int), 8), i_in = s.add(sizeof(uint32_t), n_words, occ_bits),
              i_out = s.add(sizeof(uint32_t), n_words, nullptr, occ_out);
    if ((rc = s.begin())) return rc;
    if ((rc = dilate_device(c, s.at<uint32_t>(i_in), dims, radius, s.at<uint32_t>(i_out), n_cells, s.at<int>(i_stats), n_occupied, bounds, c->stream))) return rc;
    return s.finish();
} NERF_CATCH(c)

// everything nerf_clip_rays* can refuse without a device
static int clip_check(nerf_ctx *c, const void *occ_bits, const float *lo, const float *step, const int32_t *dims, const void *origins, size_t n_origins,
                      const void *dirs, size_t n_rays, float near_, float far_, const void *bounds, const void *bounds_out, const void *hit_out) {
    const char *why = nerfclip::check_grid(occ_bits, lo, step, dims);
    if (!why) why = nerfclip::check_rays(origins, n_origins, dirs, n_rays, near_, far_, bounds, bounds_out, hit_out);
    if (why) return fail(c, NERF_ERR_INVALID, why);
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    return NERF_OK;
}

// the clip launch on device pointers; with n_hit the block sums go through BUF_CLIP and the total comes back (one synchronisation)
static int clip_device(nerf_ctx *c, const uint32_t *d_bits, const float *lo, const float *step, const int32_t *dims, const float *d_origins,
                       size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_, float far_, const float *d_bounds,
                       float *d_bounds_out, uint8_t *d_hit_out, uint64_t *n_hit, hipStream_t st) {
    ClipRaysArgs a{};
    a.bits = d_bits;
    for (int k = 0; k < 3; ++k) { a.lo[k] = lo[k]; a.step[k] = step[k]; a.dims[k] = dims[k]; }
    a.origins = d_origins; a.per_ray_origins = n_origins == 1 ? 0 : 1; a.dirs = d_dirs; a.n_rays = (int)n_rays; a.normalize = normalize ? 1 : 0;
    a.near_ = near_; a.far_ = far_; a.bounds = d_bounds; a.bounds_out = d_bounds_out; a.hit_out = d_hit_out;
    uint32_t *d_totals = nullptr;
    if (n_hit) {
        const size_t n_blocks = (n_rays + kClipBlock - 1) / kClipBlock;
        int rc;
        if ((rc = c->buf[BUF_CLIP].ensure(c, (n_blocks + 2) * sizeof(uint32_t)))) return rc;
        d_totals = c->dev<uint32_t>(BUF_CLIP);
        a.bsum = d_totals + 2;
    }
    HIP_TRY(c, launch_clip_rays(a, st));
    if (n_hit) {
        HIP_TRY(c, launch_clip_scan(a.bsum, a.n_rays, d_totals, st));
        uint32_t h[2];
        HIP_TRY(c, hipMemcpyAsync(h, d_totals, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        *n_hit = h[0];
    }
    return NERF_OK;
}

int nerf_clip_rays_device(nerf_ctx *c, const uint32_t *d_occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                          const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_, float far_,
                          const float *d_bounds, float *d_bounds_out, uint8_t *d_hit_out, uint64_t *n_hit, void *stream) try {
    int rc;
    if ((rc = clip_check(c, d_occ_bits, lo, step, dims, d_origins, n_origins, d_dirs, n_rays, near_, far_, d_bounds, d_bounds_out, d_hit_out))) return rc;
    if (n_hit) *n_hit = 0;
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    return clip_device(c, d_occ_bits, lo, step, dims, d_origins, n_origins, d_dirs, n_rays, normalize, near_, far_, d_bounds, d_bounds_out, d_hit_out,
                       n_hit, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_clip_rays(nerf_ctx *c, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3], const float *origins,
                   size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_, const float *bounds,
                   float *bounds_out, uint8_t *hit_out, uint64_t *n_hit) try {
    int rc;
    if ((rc = clip_check(c, occ_bits, lo, step, dims, origins, n_origins, dirs, n_rays, near_, far_, bounds, bounds_out, hit_out))) return rc;
    if (n_hit) *n_hit = 0;
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    // staging: occupancy, dirs, origins, [bounds], bounds_out, hit flags
    const size_t R = n_rays, n_words = ((size_t)dims[0] * dims[1] * dims[2] + 31) / 32;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_occ = s.add(sizeof(uint32_t), n_words, occ_bits), i_dirs = s.add(F, 3 * R, dirs), i_origins = s.add(F, 3 * n_origins, origins),
              i_bounds = s.opt(bounds, F, 2 * R, bounds), i_out = s.add(F, 2 * R, nullptr, bounds_out), i_hit = s.add(1, R, nullptr, hit_out);
    if ((rc = s.begin())) return rc;
    if ((rc = clip_device(c, s.at<uint32_t>(i_occ), lo, step, dims, s.at(i_origins), n_origins, s.at(i_dirs), R, normalize, near_, far_, s.at(i_bounds),
                          s.at(i_out), s.at<uint8_t>(i_hit), n_hit, c->stream))) return rc;
    return s.finish();
} NERF_CATCH(c)

// ---- isosurface meshes (isosurface_kernels.hip): marching tetrahedra on a sigma lattice -------------------------------------------------
// everything the mesh entry points can refuse without a device, in the order of density_grid_check; *n_points = dims[0] dims[1] dims[2]
static int mesh_check(nerf_ctx *c, bool from_network, int which, const void *sigma, const float *lo, const float *step, const int32_t *dims, float iso,
                      const uint64_t *n_vertices, const uint64_t *n_triangles, size_t *n_points) {
    if (from_network && which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!lo || !step || !dims) return fail(c, NERF_ERR_INVALID, "lo, step and dims must not be NULL");
    if (!from_network && !sigma) return fail(c, NERF_ERR_INVALID, "sigma must not be NULL");
    if (!n_vertices || !n_triangles) return fail(c, NERF_ERR_INVALID, "n_vertices and n_triangles are required");
    for (int k = 0; k < 3; ++k) {
        if (dims[k] < 2) return fail(c, NERF_ERR_INVALID, "dims must be at least 2 (a lattice of cells)");
        if (!std::isfinite(lo[k]) || !std::isfinite(step[k])) return fail(c, NERF_ERR_INVALID, "lo, step and iso must be finite");
        if (step[k] == 0.0f) return fail(c, NERF_ERR_INVALID, "step must not be 0");
    }
    if (!std::isfinite(iso)) return fail(c, NERF_ERR_INVALID, "lo, step and iso must be finite");
    // every count (at most 7 vertices and 12 triangles per point) fits 32 bits, and the lattice fits one launch of the grid kernel
    const size_t limit = std::min((size_t)1 << 28, c ? max_batch_points(c->n_cus) : max_batch_points(0));
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane > limit || plane * (unsigned long long)dims[2] > limit)
        return fail(c, NERF_ERR_INVALID, "lattice too large: dims[0] * dims[1] * dims[2] must be at most 2^28 (and nerf_forward_batch's largest n)");
    *n_points = (size_t)(plane * (unsigned long long)dims[2]);
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (from_network && !c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    return NERF_OK;
}

static MeshLattice mesh_lattice(const float *lo, const float *step, const int32_t *dims, float iso) {
    MeshLattice g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.step[k] = step[k]; }
    g.iso = iso;
    return g;
}

struct MeshOut { // the caller's arrays (all host or all device pointers), each optional
    float *vertices, *normals, *rgb;
    uint32_t *triangles;
    size_t cap_vertices, cap_triangles;
};

// sigma lies in the workspace: count, report both counts, and -- if an array is asked for and both counts fit -- emit.  host_out: the arrays are
// host memory (staged in the context's scratch and copied back; synchronises).  The colours are nerf_forward_batch of network colour_net at the
// vertices with dirs = -normal, run on the SoA copy the vertex kernel writes.
// Components (optional): what mesh_components prepared -- the classification then drops the points of discarded components (comp->filtered), and
// both component counts are read with the mesh's.
struct MeshComponents {
    CompWorkspace w;
    bool filtered;                    // the filter discards something in principle: classify through the keep flags
    uint64_t *n_components, *n_kept;  // the caller's, optional
};

static int mesh_extract(nerf_ctx *c, int colour_net, const MeshLattice &g, const MeshWorkspace &w, const MeshOut &o, bool host_out, uint64_t *n_vertices,
                        uint64_t *n_triangles, hipStream_t st, const MeshComponents *comp = nullptr) {
    if (comp && comp->filtered) HIP_TRY(c, launch_mesh_count(g, w, st, comp->w.label, comp->w.size));
    else HIP_TRY(c, launch_mesh_count(g, w, st));
    uint32_t totals[2] = {0, 0}, counts[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    if (comp) HIP_TRY(c, hipMemcpyAsync(counts, comp->w.counts, sizeof counts, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (comp && comp->n_components) *comp->n_components = counts[0];
    if (comp && comp->n_kept) *comp->n_kept = counts[1];
    const size_t nv = totals[0], nt = totals[1];
    *n_vertices = nv; *n_triangles = nt;
    if (!(o.vertices || o.normals || o.rgb || o.triangles) || nv > o.cap_vertices || nt > o.cap_triangles || nv == 0) return NERF_OK;
    // staging in the scratch: what the caller cannot receive directly, and the inputs / sigma output of the colour launch
    Staging s(c, BUF_SCRATCH, st);
    const int i_v = s.opt(host_out && o.vertices, F, 3 * nv, nullptr, o.vertices), i_n = s.opt(host_out && o.normals, F, 3 * nv, nullptr, o.normals),
              i_c = s.opt(host_out && o.rgb, F, 3 * nv, nullptr, o.rgb), i_t = s.opt(host_out && o.triangles, sizeof(uint32_t), 3 * nt, nullptr, o.triangles),
              i_soa = s.opt(o.rgb, F, 3 * nv), i_dir = s.opt(o.rgb, F, 3 * nv), i_sig = s.opt(o.rgb, F, nv);
    int rc;
    if ((rc = s.begin())) return rc;
    float *d_v = host_out ? s.at(i_v) : o.vertices, *d_n = host_out ? s.at(i_n) : o.normals, *d_c = host_out ? s.at(i_c) : o.rgb;
    uint32_t *d_t = host_out ? s.at<uint32_t>(i_t) : o.triangles;
    HIP_TRY(c, launch_mesh_emit(g, w, (uint32_t)nv, d_v, d_n, s.at(i_soa), s.at(i_dir), (uint32_t)nt, d_t, st));
    if (o.rgb && (rc = forward_device(c, colour_net, NERF_MLP_F32, s.at(i_soa), s.at(i_dir), nv, d_c, s.at(i_sig), st))) return rc;
    return host_out ? s.finish() : NERF_OK;
}

// ---- lattice components (components_kernels.hip) -----------------------------------------------------------------------------------------------
static int filter_check(nerf_ctx *c, const nerf_component_filter *f) {
    if (f && f->keep_largest > (uint32_t)kCompMaxRank) return fail(c, NERF_ERR_INVALID, "filter: keep_largest must be at most 64");
    return NERF_OK;
}

// the component workspace for n points (the root list and the rank map borrow the mesh workspace's prefix-sum arrays, idle at this point) and the
// labelling launches on d_sigma; the mesh workspace must have been ensured by the caller (it may hold sigma already)
static int components_launch(nerf_ctx *c, const float *d_sigma, const int32_t *dims, float iso, size_t n, uint32_t keep_largest, uint32_t min_points,
                             uint32_t cap_table, CompWorkspace *out, hipStream_t st) {
    int rc;
    if ((rc = c->buf[BUF_COMP].ensure(c, comp_workspace_bytes(n)))) return rc;
    const MeshWorkspace mw = mesh_workspace_carve(c->buf[BUF_MESH].p, n);
    *out = comp_workspace_carve(c->buf[BUF_COMP].p, n, mw.vbase, mw.tbase);
    HIP_TRY(c, launch_components(d_sigma, dims[0], dims[1], dims[2], iso, *out, keep_largest, min_points, cap_table, st));
    return NERF_OK;
}

// a filtered mesh call: label the lattice in w.sigma when the filter can discard something or a count is asked for.  *use = whether anything ran.
static int mesh_components(nerf_ctx *c, const MeshWorkspace &w, const int32_t *dims, float iso, size_t n, const nerf_component_filter *f,
                           uint64_t *n_components, uint64_t *n_kept, MeshComponents *mc, bool *use, hipStream_t st) {
    const uint32_t keep_largest = f ? f->keep_largest : 0u, min_points = f ? f->min_points : 0u;
    mc->filtered = keep_largest != 0 || min_points > 1; // every component has at least one point
    mc->n_components = n_components; mc->n_kept = n_kept;
    *use = mc->filtered || n_components || n_kept;
    if (!*use) return NERF_OK;
    return components_launch(c, w.sigma, dims, iso, n, keep_largest, min_points, 0, &mc->w, st);
}

int nerf_isosurface_grid_filtered(nerf_ctx *c, const float *sigma, const float lo[3], const float step[3], const int32_t dims[3], float iso,
                                  const void *filter, float *vertices, float *normals, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles,
                                  uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_components, uint64_t *n_kept) try {
    size_t n = 0;
    int rc;
    if ((rc = filter_check(c, (const nerf_component_filter *)filter))) return rc;
    if ((rc = mesh_check(c, false, 0, sigma, lo, step, dims, iso, n_vertices, n_triangles, &n))) return rc;
    DeviceGuard dg(c->device);
    if ((rc = c->buf[BUF_MESH].ensure(c, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace w = mesh_workspace_carve(c->buf[BUF_MESH].p, n);
    HIP_TRY(c, hipMemcpyAsync(w.sigma, sigma, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MeshComponents mc{};
    bool use = false;
    if ((rc = mesh_components(c, w, dims, iso, n, (const nerf_component_filter *)filter, n_components, n_kept, &mc, &use, c->stream))) return rc;
    const MeshOut o{vertices, normals, nullptr, triangles, cap_vertices, cap_triangles};
    return mesh_extract(c, -1, mesh_lattice(lo, step, dims, iso), w, o, true, n_vertices, n_triangles, c->stream, use ? &mc : nullptr);
} NERF_CATCH(c)

int nerf_isosurface_grid(nerf_ctx *c, const float *sigma, const float lo[3], const float step[3], const int32_t dims[3], float iso, float *vertices,
                         float *normals, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles) {
    return nerf_isosurface_grid_filtered(c, sigma, lo, step, dims, iso, nullptr, vertices, normals, cap_vertices, triangles, cap_triangles, n_vertices,
                                         n_triangles, nullptr, nullptr);
}

// everything nerf_lattice_components* can refuse without a device; *n_points = dims[0] dims[1] dims[2]
static int components_check(nerf_ctx *c, const void *sigma, const int32_t *dims, float iso, const void *table, size_t cap_table, const uint64_t *n_components,
                            size_t *n_points) {
    if (!sigma) return fail(c, NERF_ERR_INVALID, "sigma must not be NULL");
    if (!dims) return fail(c, NERF_ERR_INVALID, "dims must not be NULL");
    if (!n_components) return fail(c, NERF_ERR_INVALID, "n_components is required");
    for (int k = 0; k < 3; ++k)
        if (dims[k] < 1) return fail(c, NERF_ERR_INVALID, "dims must be positive");
    if (!std::isfinite(iso)) return fail(c, NERF_ERR_INVALID, "iso must be finite");
    if (cap_table > (size_t)kCompMaxRank) return fail(c, NERF_ERR_INVALID, "cap_table must be at most 64");
    if (table && cap_table == 0) return fail(c, NERF_ERR_INVALID, "a table needs cap_table > 0");
    const size_t limit = std::min((size_t)1 << 28, c ? max_batch_points(c->n_cus) : max_batch_points(0));
    const unsigned long long plane = (unsigned long long)dims[0] * (unsigned long long)dims[1];
    if (plane > limit || plane * (unsigned long long)dims[2] > limit)
        return fail(c, NERF_ERR_INVALID, "lattice too large: dims[0] * dims[1] * dims[2] must be at most 2^28 (and nerf_forward_batch's largest n)");
    *n_points = (size_t)(plane * (unsigned long long)dims[2]);
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    return NERF_OK;
}

// labels of d_sigma; labels_out is host (staged through the workspace's own label array) or device memory.  Synchronises st.
static int lattice_components(nerf_ctx *c, const float *d_sigma, const int32_t *dims, float iso, size_t n, uint32_t *labels_out, bool host_out,
                              nerf_component *table, size_t cap_table, uint64_t *n_components, hipStream_t st) {
    static_assert(sizeof(nerf_component) == sizeof(CompEntry) && sizeof(nerf_component) == 32 && sizeof(nerf_component_filter) == 8, "component structs");
    int rc;
    CompWorkspace w;
    const uint32_t cap = table ? (uint32_t)cap_table : 0u;
    if ((rc = components_launch(c, d_sigma, dims, iso, n, 0, 0, cap, &w, st))) return rc;
    uint32_t counts[2] = {0, 0};
    CompEntry entries[kCompMaxRank];
    HIP_TRY(c, hipMemcpyAsync(counts, w.counts, sizeof counts, hipMemcpyDeviceToHost, st));
    if (cap) HIP_TRY(c, hipMemcpyAsync(entries, w.table, cap * sizeof(CompEntry), hipMemcpyDeviceToHost, st));
    if (labels_out) HIP_TRY(c, hipMemcpyAsync(labels_out, w.label, n * sizeof(uint32_t), host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *n_components = counts[0];
    const size_t filled = std::min((size_t)cap, (size_t)counts[0]);
    if (filled) memcpy(table, entries, filled * sizeof(CompEntry));
    return NERF_OK;
}

int nerf_lattice_components(nerf_ctx *c, const float *sigma, const int32_t dims[3], float iso, uint32_t *labels_out, void *table, size_t cap_table,
                            uint64_t *n_components) try {
    size_t n = 0;
    int rc;
    if ((rc = components_check(c, sigma, dims, iso, table, cap_table, n_components, &n))) return rc;
    DeviceGuard dg(c->device);
    if ((rc = c->buf[BUF_MESH].ensure(c, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace mw = mesh_workspace_carve(c->buf[BUF_MESH].p, n);
    HIP_TRY(c, hipMemcpyAsync(mw.sigma, sigma, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return lattice_components(c, mw.sigma, dims, iso, n, labels_out, true, (nerf_component *)table, cap_table, n_components, c->stream);
} NERF_CATCH(c)

int nerf_lattice_components_device(nerf_ctx *c, const float *d_sigma, const int32_t dims[3], float iso, uint32_t *d_labels_out, void *table, size_t cap_table,
                                   uint64_t *n_components, void *stream) try {
    size_t n = 0;
    int rc;
    if ((rc = components_check(c, d_sigma, dims, iso, table, cap_table, n_components, &n))) return rc;
    DeviceGuard dg(c->device);
    if ((rc = c->buf[BUF_MESH].ensure(c, mesh_workspace_bytes(n)))) return rc;
    return lattice_components(c, d_sigma, dims, iso, n, d_labels_out, false, (nerf_component *)table, cap_table, n_components, (hipStream_t)stream);
} NERF_CATCH(c)

// sigma of network `which` in grid mode into the workspace, then the kernels of nerf_isosurface_grid
static int extract_mesh(nerf_ctx *c, int which, const float *lo, const float *step, const int32_t *dims, float iso, const MeshOut &o, bool host_out,
                        uint64_t *n_vertices, uint64_t *n_triangles, hipStream_t st, const nerf_component_filter *filter = nullptr,
                        uint64_t *n_components = nullptr, uint64_t *n_kept = nullptr) {
    size_t n = 0;
    int rc;
    if ((rc = filter_check(c, filter))) return rc;
    if ((rc = mesh_check(c, true, which, nullptr, lo, step, dims, iso, n_vertices, n_triangles, &n))) return rc;
    DeviceGuard dg(c->device);
    if ((rc = c->buf[BUF_MESH].ensure(c, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace w = mesh_workspace_carve(c->buf[BUF_MESH].p, n);
    if ((rc = density_grid_launch(c, which, lo, step, dims, n, w.sigma, 0.0f, nullptr, nullptr, st))) return rc;
    MeshComponents mc{};
    bool use = false;
    if ((rc = mesh_components(c, w, dims, iso, n, filter, n_components, n_kept, &mc, &use, st))) return rc;
    return mesh_extract(c, which, mesh_lattice(lo, step, dims, iso), w, o, host_out, n_vertices, n_triangles, st, use ? &mc : nullptr);
}

int nerf_extract_mesh_filtered(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso, const void *filter,
                               float *vertices, float *normals, float *rgb, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles,
                               uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_components, uint64_t *n_kept) try {
    const MeshOut o{vertices, normals, rgb, triangles, cap_vertices, cap_triangles};
    return extract_mesh(c, which, lo, step, dims, iso, o, true, n_vertices, n_triangles, c ? c->stream : nullptr, (const nerf_component_filter *)filter,
                        n_components, n_kept);
} NERF_CATCH(c)

int nerf_extract_mesh_filtered_device(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso, const void *filter,
                                      float *d_vertices, float *d_normals, float *d_rgb, size_t cap_vertices, uint32_t *d_triangles, size_t cap_triangles,
                                      uint64_t *n_vertices, uint64_t *n_triangles, uint64_t *n_components, uint64_t *n_kept, void *stream) try {
    const MeshOut o{d_vertices, d_normals, d_rgb, d_triangles, cap_vertices, cap_triangles};
    return extract_mesh(c, which, lo, step, dims, iso, o, false, n_vertices, n_triangles, (hipStream_t)stream, (const nerf_component_filter *)filter,
                        n_components, n_kept);
} NERF_CATCH(c)

int nerf_extract_mesh(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso, float *vertices, float *normals,
                      float *rgb, size_t cap_vertices, uint32_t *triangles, size_t cap_triangles, uint64_t *n_vertices, uint64_t *n_triangles) try {
    const MeshOut o{vertices, normals, rgb, triangles, cap_vertices, cap_triangles};
    return extract_mesh(c, which, lo, step, dims, iso, o, true, n_vertices, n_triangles, c ? c->stream : nullptr);
} NERF_CATCH(c)

int nerf_extract_mesh_device(nerf_ctx *c, int which, const float lo[3], const float step[3], const int32_t dims[3], float iso, float *d_vertices,
                             float *d_normals, float *d_rgb, size_t cap_vertices, uint32_t *d_triangles, size_t cap_triangles, uint64_t *n_vertices,
                             uint64_t *n_triangles, void *stream) try {
    const MeshOut o{d_vertices, d_normals, d_rgb, d_triangles, cap_vertices, cap_triangles};
    return extract_mesh(c, which, lo, step, dims, iso, o, false, n_vertices, n_triangles, (hipStream_t)stream);
} NERF_CATCH(c)

// ---- density gradients at caller points (normal_kernels.hip around the sigma-only launch) -----------------------------------------------
// The points run in chunks of at most c->gradient_chunk (and of what one MLP launch takes for six stencil points each): per chunk
// stencil -> sigma-only MLP over 6 m points -> combine, all on `st`, nothing comes back to the host.  A point's gradient depends on that
// point alone (the sigma-only kernel's bits do not depend on the slot), so the chunking shows in no bit.
// what nerf_density_gradient_batch* refuses, in its order; n == 0 passes here and makes the caller return at once
static int density_gradient_check(nerf_ctx *c, int which, const void *pts, size_t n, float h, const void *grad) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!(std::isfinite(h) && h > 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and greater than 0");
    if (n > 0 && (!pts || !grad)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    return NERF_OK;
}

static int density_gradient_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float h, float *d_grad, hipStream_t st) {
    int rc;
    if ((rc = density_gradient_check(c, which, d_pts, n, h, d_grad)) || n == 0) return rc;
    DeviceGuard dg(c->device);
    const size_t chunk = std::max<size_t>(1, std::min({c->gradient_chunk, n, max_batch_points(c->n_cus) / 6}));
    if ((rc = c->buf[BUF_STENCIL].ensure(c, 6 * chunk * 4 * sizeof(float)))) return rc;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        float *d_spts = c->dev(BUF_STENCIL), *d_ssig = d_spts + 18 * m;
        NormalStencilArgs sa{};
        sa.n_live = (uint32_t)m; sa.h = h; sa.src = d_pts + i0; sa.src_stride = n; sa.pts = d_spts;
        HIP_TRY(c, launch_normal_stencil(sa, st));
        HIP_TRY(c, launch_sigma_points(c, c->net[which], d_spts, 6 * m, d_ssig, st));
        NormalCombineArgs ca{(uint32_t)m, d_spts, d_ssig, d_grad + i0, n};
        HIP_TRY(c, launch_normal_combine(ca, st));
    }
    return NERF_OK;
}

int nerf_density_gradient_batch_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float h, float *d_grad, void *stream) try {
    return density_gradient_device(c, which, d_pts, n, h, d_grad, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_density_gradient_batch(nerf_ctx *c, int which, const float *pts, size_t n, float h, float *grad) try {
    int rc;
    if ((rc = density_gradient_check(c, which, pts, n, h, grad)) || n == 0) return rc;
    DeviceGuard dg(c->device);
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_pts = s.add(F, 3 * n, pts), i_grad = s.add(F, 3 * n, nullptr, grad);
    if ((rc = s.begin())) return rc;
    if ((rc = density_gradient_device(c, which, s.at(i_pts), n, h, s.at(i_grad), c->stream))) return rc;
    return s.finish();
} NERF_CATCH(c)

// ---- stage entry points ------------------------------------------------------------------------------------
static int stage_rect(nerf_ctx *c, const nerf_camera *cam, int x0, int y0, int w, int h, RayGenArgs &g) {
    int rc;
    if ((rc = check_camera(c, cam))) return rc;
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 + w > cam->nx || y0 + h > cam->ny) return fail(c, NERF_ERR_INVALID, "rectangle outside the frame");
    g = make_raygen(*cam, 1);
    g.n_rays = w * h; g.rx0 = x0; g.ry0 = y0; g.rw = w;
    return NERF_OK;
}

int nerf_stage_ray_dirs(nerf_ctx *c, const nerf_camera *cam, int x0, int y0, int w, int h, int normalize, float *out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    DeviceGuard dg(c->device);
    RayGenArgs g; int rc;
    if ((rc = stage_rect(c, cam, x0, y0, w, h, g))) return rc;
    g.normalize = normalize ? 1 : 0;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_out = s.add(F, (size_t)g.n_rays * 3, nullptr, out);
    if ((rc = s.begin())) return rc;
    HIP_TRY(c, launch_ray_dirs(g, s.at(i_out), c->stream));
    return s.finish();
} NERF_CATCH(c)

int nerf_stage_stratified(nerf_ctx *c, const nerf_camera *cam, int x0, int y0, int w, int h, int count, uint64_t seed, float *out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (count <= 0) return NERF_OK; // src/lib.rs:235-237
    DeviceGuard dg(c->device);
    RayGenArgs g; int rc;
    if ((rc = stage_rect(c, cam, x0, y0, w, h, g))) return rc;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_out = s.add(F, (size_t)g.n_rays * count, nullptr, out);
    if ((rc = s.begin())) return rc;
    HIP_TRY(c, launch_stratified(g, count, cam->near_, cam->far_, seed, s.at(i_out), c->stream));
    return s.finish();
} NERF_CATCH(c)

static int stage_resample(nerf_ctx *c, size_t n_rays, int nc, int nf, float far_, uint64_t seed, const uint32_t *pixel_index,
                          const float *t_coarse, const float *sigma_coarse, const float *u, float *w_out, float *cdf_out,
                          float *t_new_out, float *t_fine_out, float tau, uint8_t *flags_out) {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays == 0) return NERF_OK;
    if (!t_coarse || !sigma_coarse || (!t_fine_out && !flags_out)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (nc < 3 || nf <= 0) return fail(c, NERF_ERR_INVALID, "resample needs nc >= 3 and nf > 0 (src/lib.rs:295-297)");
    if (!u && !pixel_index) return fail(c, NERF_ERR_INVALID, "either u or pixel_index must be given");
    if (resample_lds_bytes(nc, nf) > 160 * 1024 || n_rays > 0x7fffffff / (size_t)(nc + nf)) return fail(c, NERF_ERR_INVALID, "too many samples");
    DeviceGuard dg(c->device);
    const size_t R = n_rays, M = (size_t)nc + nf;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_tc = s.add(F, R * nc, t_coarse), i_sc = s.add(F, R * nc, sigma_coarse), i_u = s.opt(u, F, R * nf, u), i_w = s.add(F, R * nc, nullptr, w_out),
              i_cdf = s.add(F, R * (nc - 1), nullptr, cdf_out), i_tn = s.add(F, R * nf, nullptr, t_new_out), i_tf = s.add(F, R * M, nullptr, t_fine_out),
              i_px = s.opt(pixel_index, sizeof(uint32_t), R, pixel_index), i_fl = s.opt(flags_out, 1, R, nullptr, flags_out);
    int rc;
    if ((rc = s.begin())) return rc;
    ResampleArgs ra{};
    ra.n_rays = (int)R; ra.nc = nc; ra.nf = nf; ra.far_ = far_;
    ra.seed_lo = (uint32_t)seed; ra.seed_hi = (uint32_t)(seed >> 32);
    ra.t_coarse = s.at(i_tc); ra.sigma_coarse = s.at(i_sc); ra.t_fine = s.at(i_tf);
    ra.pixel_index = s.at<uint32_t>(i_px); ra.u_in = s.at(i_u);
    ra.w_out = s.at(i_w); ra.cdf_out = s.at(i_cdf); ra.t_new_out = s.at(i_tn);
    ra.g.rw = 1; ra.g.rnx = 1; // unused when pixel_index/u are given
    if (flags_out) { ra.flag_tau = tau; ra.flag_out = s.at<unsigned char>(i_fl); }
    HIP_TRY(c, launch_resample(ra, c->stream));
    return s.finish();
}

int nerf_stage_resample(nerf_ctx *c, size_t n_rays, int nc, int nf, float far_, uint64_t seed, const uint32_t *pixel_index,
                        const float *t_coarse, const float *sigma_coarse, const float *u, float *w_out, float *cdf_out,
                        float *t_new_out, float *t_fine_out) try {
    return stage_resample(c, n_rays, nc, nf, far_, seed, pixel_index, t_coarse, sigma_coarse, u, w_out, cdf_out, t_new_out, t_fine_out, 0.0f, nullptr);
} NERF_CATCH(c)

int nerf_stage_hybrid_flags(nerf_ctx *c, size_t n_rays, int nc, int nf, float far_, uint64_t seed, const uint32_t *pixel_index,
                            const float *t_coarse, const float *sigma_coarse, const float *u, float tau, uint8_t *flags_out,
                            float *t_new_out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays && !flags_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!(tau >= 0.0f)) return fail(c, NERF_ERR_INVALID, "tau must be >= 0 (0 selects the context's threshold)");
    return stage_resample(c, n_rays, nc, nf, far_, seed, pixel_index, t_coarse, sigma_coarse, u, nullptr, nullptr, t_new_out, nullptr,
                          tau > 0.0f ? tau : c->hybrid_tau, flags_out);
} NERF_CATCH(c)

// the order kernel over a caller's t: the table, the per-block flags, or both
static int stage_depth_order(nerf_ctx *c, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *table_out, uint32_t *flags_out) {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!t || (!table_out && !flags_out)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (rows <= 0 || rays_per_row <= 0 || samples_per_ray <= 0 || (long long)rows * rays_per_row * samples_per_ray > 0x3fffffff)
        return fail(c, NERF_ERR_INVALID, "rows, rays_per_row and samples_per_ray must be > 0 and within one pass");
    const int n = rows * rays_per_row * samples_per_ray;
    const nerfmlp::DepthOrder d = nerfmlp::depth_order_of(n, samples_per_ray, rays_per_row, true, true); // as the full launch of an image pass of this shape
    if (d.tiles == 0) return fail(c, NERF_ERR_INVALID, "this window is not depth-ordered: rays_per_row % 8 == 0, rows >= 4, samples_per_ray % 32 == 0 and <= 512");
    DeviceGuard dg(c->device);
    int rc;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_t = s.add(F, (size_t)n, t), i_table = s.add(sizeof(uint32_t), (size_t)d.points, nullptr, table_out);
    const int i_flags = flags_out ? s.add(sizeof(uint32_t), (size_t)d.blocks, nullptr, flags_out) : -1;
    if ((rc = s.begin())) return rc;
    DepthOrderArgs q{};
    q.t = s.at(i_t); q.rw = rays_per_row; q.spr = samples_per_ray; q.blocks_x = d.blocks_x; q.blocks = d.blocks; q.table = s.at<unsigned int>(i_table);
    if (flags_out) q.flags = s.at<unsigned int>(i_flags);
    HIP_TRY(c, launch_depth_order(q, c->stream));
    return s.finish();
}

int nerf_stage_depth_order(nerf_ctx *c, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *table_out) try {
    if (c && !table_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    return stage_depth_order(c, rows, rays_per_row, samples_per_ray, t, table_out, nullptr);
} NERF_CATCH(c)

int nerf_stage_depth_order_flags(nerf_ctx *c, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *flags_out) try {
    if (c && !flags_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    return stage_depth_order(c, rows, rays_per_row, samples_per_ray, t, nullptr, flags_out);
} NERF_CATCH(c)

int nerf_stage_integrate(nerf_ctx *c, size_t n_rays, int n, float far_, const float *rgb, const float *sigma, const float *t,
                         float *rgb_out, float *w_out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays == 0) return NERF_OK;
    if (!rgb_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (n == 0) { memset(rgb_out, 0, n_rays * 3 * sizeof(float)); return NERF_OK; } // src/lib.rs:178-180
    if (n < 0 || !rgb || !sigma || !t) return fail(c, NERF_ERR_INVALID, "bad argument");
    if (composite_lds_bytes(n) > 160 * 1024 || n_rays > 0x7fffffff / (size_t)n) return fail(c, NERF_ERR_INVALID, "too many samples");
    DeviceGuard dg(c->device);
    const size_t R = n_rays, N = (size_t)n;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_t = s.add(F, R * N, t), i_s = s.add(F, R * N, sigma), i_c = s.add(F, 3 * R * N, rgb), i_w = s.add(F, R * N, nullptr, w_out),
              i_o = s.add(F, 3 * R, nullptr, rgb_out);
    int rc;
    if ((rc = s.begin())) return rc;
    CompositeArgs ca{};
    ca.n_rays = (int)R; ca.n = n; ca.far_ = far_; ca.t = s.at(i_t); ca.sigma = s.at(i_s); ca.rgb = s.at(i_c); ca.out = s.at(i_o); ca.w_out = s.at(i_w);
    HIP_TRY(c, launch_composite(ca, c->stream));
    return s.finish();
} NERF_CATCH(c)

int nerf_stage_integrate_rgba8(nerf_ctx *c, size_t n_rays, int n, float far_, const float *rgb, const float *sigma, const float *t,
                               const float background[3], int alpha_mode, uint8_t *rgba_out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    int rc;
    const float *bg = nullptr;
    if ((rc = check_rgba8(c, background, alpha_mode, rgba_out, &bg))) return rc;
    if (n_rays == 0) return NERF_OK;
    if (n <= 0 || !rgb || !sigma || !t) return fail(c, NERF_ERR_INVALID, "bad argument");
    if (composite_lds_bytes(n) > 160 * 1024 || n_rays > 0x7fffffff / (size_t)n) return fail(c, NERF_ERR_INVALID, "too many samples");
    DeviceGuard dg(c->device);
    const size_t R = n_rays, N = (size_t)n;
    // per-ray colour, [per-ray opacity] and the packed words behind the inputs
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_t = s.add(F, R * N, t), i_s = s.add(F, R * N, sigma), i_c = s.add(F, 3 * R * N, rgb), i_o = s.add(F, 3 * R),
              i_a = s.opt(alpha_mode != NERF_ALPHA_OPAQUE, F, R), i_p = s.add(4, R, nullptr, rgba_out);
    if ((rc = s.begin())) return rc;
    CompositeArgs ca{};
    ca.n_rays = (int)R; ca.n = n; ca.far_ = far_; ca.t = s.at(i_t); ca.sigma = s.at(i_s); ca.rgb = s.at(i_c); ca.out = s.at(i_o); ca.opacity = s.at(i_a);
    if (bg) { ca.use_bg = 1; ca.bg[0] = bg[0]; ca.bg[1] = bg[1]; ca.bg[2] = bg[2]; }
    HIP_TRY(c, launch_composite(ca, c->stream));
    HIP_TRY(c, launch_pack_rgba8(ca.out, ca.opacity, s.at<uint32_t>(i_p), R, alpha_mode, c->stream));
    return s.finish();
} NERF_CATCH(c)

// ---- certify_zero's device pieces on caller data (cert_pass's launches, one at a time) ---------------------------------------------
// A list or aux buffer leaves as the device held it: kStageGuard words in front, the entries, kStageGuard words behind, all of them
// 0xFFFFFFFF before the launch -- a word the kernel did not write still reads 0xFFFFFFFF, inside the capacity or outside.
constexpr size_t kStageGuard = NERF_STAGE_GUARD_WORDS;

// what the three list stages refuse without a device, in this order; *n = n_rays * spr
static int cert_shape_check(nerf_ctx *c, size_t n_rays, int spr, size_t lds_bytes, size_t lds_max, uint32_t list_capacity, size_t *n) {
    if (spr <= 0) return fail(c, NERF_ERR_INVALID, "spr must be positive");
    if (lds_bytes > lds_max) return fail(c, NERF_ERR_INVALID, "too many samples per ray");
    if (n_rays > (size_t)0x7fffffff / (size_t)spr) return fail(c, NERF_ERR_INVALID, "too many samples (a list entry holds 31 index bits)");
    *n = n_rays * (size_t)spr;
    if (list_capacity > *n) return fail(c, NERF_ERR_INVALID, "list_capacity exceeds n_rays * spr");
    return NERF_OK;
}

static bool low_bit_mask(uint32_t m) { return (m & (m + 1u)) == 0u; } // 2^k - 1

int nerf_stage_cert_plan(nerf_ctx *c, size_t n_rays, int spr, float far_, float margin, float depth_limit, uint32_t audit_mask,
                         uint32_t audit_mask_near, uint32_t audit_salt, int back_part, float zero_threshold, uint32_t list_capacity,
                         uint32_t aux_capacity, const float *t, float *pre, int32_t *jstar_out, uint32_t *list_out, uint32_t *counts_out,
                         uint32_t *aux_out, int32_t *rays_per_wave_out) try {
    size_t N = 0;
    int rc, rpw = 0;
    const size_t lds = spr > 0 ? cert_plan_lds_bytes(spr, &rpw) : 0;
    if ((rc = cert_shape_check(c, n_rays, spr, lds, (size_t)159 * 1024, list_capacity, &N))) return rc;
    if (aux_capacity > N) return fail(c, NERF_ERR_INVALID, "aux_capacity exceeds n_rays * spr");
    if (!(margin >= 0.0f) || !(margin <= 3.0e38f)) return fail(c, NERF_ERR_INVALID, "margin must be finite and >= 0");
    if (back_part && !(zero_threshold == zero_threshold)) return fail(c, NERF_ERR_INVALID, "zero_threshold is NaN");
    if (depth_limit != depth_limit) return fail(c, NERF_ERR_INVALID, "depth_limit is NaN");
    if (!low_bit_mask(audit_mask) || !low_bit_mask(audit_mask_near)) return fail(c, NERF_ERR_INVALID, "an audit mask must be 2^k - 1");
    if (!t || !pre || !jstar_out || !list_out || !counts_out || !aux_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (rays_per_wave_out) *rays_per_wave_out = rpw;
    counts_out[0] = counts_out[1] = counts_out[2] = 0;
    const size_t n_list = list_capacity + 2 * kStageGuard, n_aux = 2 * (size_t)aux_capacity + 2 * kStageGuard;
    memset(list_out, 0xFF, n_list * 4);
    memset(aux_out, 0xFF, n_aux * 4);
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    // pre, t, jstar, the three counters, the guarded list and the guarded aux records (each guarded region one part)
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_pre = s.add(4, N, pre, pre), i_t = s.add(4, N, t), i_j = s.add(4, n_rays, nullptr, jstar_out, 0xFF), i_cnt = s.add(4, 3, nullptr, counts_out, 0x00),
              i_list = s.add(4, n_list, nullptr, list_out, 0xFF), i_aux = s.add(4, n_aux, nullptr, aux_out, 0xFF);
    if ((rc = s.begin())) return rc;
    uint32_t *cnt = s.at<uint32_t>(i_cnt);
    CertPlanArgs q{};
    q.pre = s.at(i_pre); q.t = s.at(i_t); q.n_rays = (int)n_rays; q.spr = spr; q.far_ = far_;
    q.margin = margin; q.depth_limit = depth_limit; q.audit_mask = audit_mask; q.audit_mask_near = audit_mask_near; q.audit_salt = audit_salt;
    q.list = s.at<uint32_t>(i_list) + kStageGuard; q.count = cnt; q.capacity = list_capacity; q.jstar = s.at<int>(i_j);
    if (back_part) { q.count_back = cnt + 1; q.zero_threshold = zero_threshold; }
    q.aux = s.at<uint32_t>(i_aux) + kStageGuard; q.aux_count = cnt + 2; q.aux_capacity = aux_capacity;
    HIP_TRY(c, launch_cert_plan(q, c->stream));
    return s.finish();
} NERF_CATCH(c)

int nerf_stage_cert_verify(nerf_ctx *c, size_t n_rays, int spr, float far_, uint32_t list_capacity, const float *t, const int32_t *jstar,
                           float *sigma, uint32_t *list_out, uint32_t *count, uint32_t *fallback_rays) try {
    size_t N = 0;
    int rc;
    if ((rc = cert_shape_check(c, n_rays, spr, spr > 0 ? (size_t)4 * spr * sizeof(float) : 0, (size_t)160 * 1024, list_capacity, &N))) return rc;
    if (!t || !jstar || !sigma || !list_out || !count || !fallback_rays) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    for (size_t r = 0; r < n_rays; ++r)
        if (jstar[r] < 0 || jstar[r] > spr) return fail(c, NERF_ERR_INVALID, "jstar must lie in [0, spr]");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    const size_t n_list = list_capacity + 2 * kStageGuard;
    memset(list_out, 0xFF, n_list * 4);
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    // sigma, t, jstar, {count, fall-back rays}, the guarded list (one part)
    uint32_t cnt[2] = {*count, *fallback_rays};
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_s = s.add(4, N, sigma, sigma), i_t = s.add(4, N, t), i_j = s.add(4, n_rays, jstar), i_cnt = s.add(4, 2, cnt, cnt),
              i_list = s.add(4, n_list, nullptr, list_out, 0xFF);
    if ((rc = s.begin())) return rc;
    CertVerifyArgs v{};
    v.t = s.at(i_t); v.sigma = s.at(i_s); v.n_rays = (int)n_rays; v.spr = spr; v.far_ = far_; v.jstar = s.at<int>(i_j);
    v.list = s.at<uint32_t>(i_list) + kStageGuard; v.count = s.at<uint32_t>(i_cnt); v.capacity = list_capacity; v.fallback_rays = v.count + 1;
    HIP_TRY(c, launch_cert_verify(v, c->stream));
    if ((rc = s.finish())) return rc;
    *count = cnt[0]; *fallback_rays = cnt[1];
    return NERF_OK;
} NERF_CATCH(c)

int nerf_stage_cert_audit(nerf_ctx *c, const uint32_t *aux, uint32_t aux_count, uint32_t aux_capacity, size_t n_sigma, float *sigma,
                          uint32_t *audit) try {
    const size_t n_rec = std::min(aux_count, aux_capacity);
    if (n_sigma > (size_t)0x7fffffff) return fail(c, NERF_ERR_INVALID, "too many samples (a list entry holds 31 index bits)");
    if (!audit || (n_rec && (!aux || !sigma))) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    for (size_t k = 0; k < n_rec; ++k)
        if (aux[2 * k] >= n_sigma) return fail(c, NERF_ERR_INVALID, "an aux record names a sample outside sigma");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    DeviceGuard dg(c->device);
    // sigma, the records, the count, the four audit words
    int rc;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_s = s.add(4, n_sigma, sigma, sigma), i_a = s.add(4, 2 * n_rec, aux), i_cnt = s.add(4, 1, &aux_count), i_w = s.add(4, 4, audit, audit);
    if ((rc = s.begin())) return rc;
    HIP_TRY(c, launch_cert_audit(s.at<uint32_t>(i_a), s.at<uint32_t>(i_cnt), aux_capacity, s.at(i_s), s.at<uint32_t>(i_w), c->n_cus, c->stream));
    return s.finish();
} NERF_CATCH(c)

} // extern "C"

// nerf_stage_prefilter (origin: one for every ray) and nerf_stage_prefilter_rays (origins: n_rays x 3, SeqArgs.ray_origins)
static int stage_prefilter(nerf_ctx *c, int which, int f16, const float *origin, const float *origins, const float *dirs, const float *t, size_t n_rays,
                           int spr, float far_, float cut_T, float *pre_out, uint32_t *nonfinite_tiles) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (spr <= 0) return fail(c, NERF_ERR_INVALID, "spr must be positive");
    if (n_rays > (size_t)0x7fffffff / (size_t)spr) return fail(c, NERF_ERR_INVALID, "too many samples");
    if (!(cut_T >= 0.0f) || !(cut_T < 1.0f)) return fail(c, NERF_ERR_INVALID, "cut_T must lie in [0, 1)");
    if ((!origin && !origins) || !dirs || !t || !pre_out || !nonfinite_tiles) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    const DevNet &net = c->net[which];
    if (!net.loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    const Prefilter &pf = prefilter_of(f16 != 0);
    if (!net.buf[pf.stream].p) return fail(c, NERF_ERR_STATE, "the f16 pre-filter is unavailable for this network: a weight exceeds the f16 range");
    *nonfinite_tiles = 0;
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    const size_t N = n_rays * (size_t)spr;
    // directions, t, pre-activations (NaN = "not evaluated", as cert_pass fills them), {ray queue, non-finite tiles, samples evaluated (64 bits)}, [origins]
    int rc;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_d = s.add(F, 3 * n_rays, dirs), i_t = s.add(F, N, t), i_p = s.add(F, N, nullptr, pre_out, 0xFF), i_cnt = s.add(4, 4, nullptr, nullptr, 0x00),
              i_o = s.opt(origins, F, 3 * n_rays, origins);
    if ((rc = s.begin())) return rc;
    uint32_t *cnt = s.at<uint32_t>(i_cnt);
    SeqArgs q{};
    q.wstream = net.at(pf.stream); q.small_params = net.at(NET_SMALL);
    q.n_rays = (int)n_rays; q.samples_per_ray = spr; q.ray_dirs = s.at(i_d); q.t = s.at(i_t); q.far_ = far_;
    if (origins) q.ray_origins = s.at(i_o);
    else copy3(q.origin, origin);
    q.sigma_out = s.at(i_p);
    q.ray_counter = cnt; q.nonfinite = cnt + 1; q.stats = (unsigned long long *)(cnt + 2);
    q.prefilter = 1; q.prefilter_cut_T = cut_T;
    HIP_TRY(c, pf.trunk(q, false, c->n_cus, c->stream));
    HIP_TRY(c, hipMemcpyAsync(nonfinite_tiles, cnt + 1, 4, hipMemcpyDeviceToHost, c->stream));
    return s.finish();
}

extern "C" {

int nerf_stage_prefilter(nerf_ctx *c, int which, int f16, const float origin[3], const float *dirs, const float *t, size_t n_rays, int spr,
                         float far_, float cut_T, float *pre_out, uint32_t *nonfinite_tiles) try {
    return stage_prefilter(c, which, f16, origin, nullptr, dirs, t, n_rays, spr, far_, cut_T, pre_out, nonfinite_tiles);
} NERF_CATCH(c)

int nerf_stage_prefilter_rays(nerf_ctx *c, int which, int f16, const float *origins, const float *dirs, const float *t, size_t n_rays, int spr,
                              float far_, float cut_T, float *pre_out, uint32_t *nonfinite_tiles) try {
    return stage_prefilter(c, which, f16, nullptr, origins, dirs, t, n_rays, spr, far_, cut_T, pre_out, nonfinite_tiles);
} NERF_CATCH(c)

// ---- the two kernels of nerf_render_rays_quantiles / nerf_render_rays_points on caller data (surface_kernels.h) ------------------------
int nerf_stage_ray_quantiles(nerf_ctx *c, size_t n_rays, int n, const float *w, const float *t, const float *quantiles, int n_q,
                             float *depth_q_out) try {
    if (n_q < 1 || n_q > NERF_MAX_QUANTILES) return fail(c, NERF_ERR_INVALID, "n_q must be between 1 and NERF_MAX_QUANTILES (8)");
    if (!quantiles) return fail(c, NERF_ERR_INVALID, "quantiles must not be NULL");
    for (int k = 0; k < n_q; ++k)
        if (!(std::isfinite(quantiles[k]) && quantiles[k] > 0.0f && quantiles[k] <= 1.0f)) return fail(c, NERF_ERR_INVALID, "a quantile must be finite and lie in (0, 1]");
    if (n <= 0) return fail(c, NERF_ERR_INVALID, "n must be positive");
    if (n_rays > (size_t)0x7fffffff / (size_t)n) return fail(c, NERF_ERR_INVALID, "too many samples");
    if (n_rays > 0 && (!w || !t || !depth_q_out)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    const size_t R = n_rays, N = (size_t)n;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_w = s.add(F, R * N, w), i_t = s.add(F, R * N, t), i_o = s.add(F, (size_t)n_q * R, nullptr, depth_q_out);
    int rc;
    if ((rc = s.begin())) return rc;
    RayQuantileArgs a{};
    a.n_rays = (int)R; a.n = n; a.w = s.at(i_w); a.t = s.at(i_t); a.n_q = n_q;
    for (int k = 0; k < n_q; ++k) a.q[k] = quantiles[k];
    a.out = s.at(i_o); a.plane_stride = R;
    HIP_TRY(c, launch_ray_quantiles(a, c->stream));
    return s.finish();
} NERF_CATCH(c)

// Every output array holds `capacity` records and NERF_STAGE_GUARD_WORDS words behind them, all 0xFFFFFFFF before the launches, and comes
// back as the device held it: a word the kernels did not write still reads 0xFFFFFFFF.
int nerf_stage_gather_points(nerf_ctx *c, size_t n_rays, const float *origins, size_t n_origins, const float *dirs, const float *depth_q,
                             const float *premultiplied_rgb, const float *opacity, const float *normals, float min_opacity, size_t capacity,
                             float *xyz_out, float *rgb_out, float *normals_out, uint32_t *ray_out, float *depth_out, float *opacity_out,
                             size_t *n_points) try {
    if (n_rays > (size_t)0x7fffffff) return fail(c, NERF_ERR_INVALID, "n_rays must be at most INT32_MAX");
    if (n_origins != 1 && n_origins != n_rays) return fail(c, NERF_ERR_INVALID, "n_origins must be 1 (one origin for every ray) or n_rays");
    if (!(std::isfinite(min_opacity) && min_opacity >= 0.0f && min_opacity <= 1.0f)) return fail(c, NERF_ERR_INVALID, "min_opacity must be finite and lie in [0, 1]");
    if (capacity > (size_t)0x7fffffff) return fail(c, NERF_ERR_INVALID, "capacity must be at most INT32_MAX");
    if (n_rays > 0 && (!origins || !dirs || !depth_q || !premultiplied_rgb || !opacity)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!xyz_out || !rgb_out || !n_points) return fail(c, NERF_ERR_INVALID, "xyz_out, rgb_out and n_points must not be NULL");
    if ((normals != nullptr) != (normals_out != nullptr)) return fail(c, NERF_ERR_INVALID, "normals and normals_out go together");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    *n_points = 0;
    DeviceGuard dg(c->device);
    const size_t R = n_rays, G = kStageGuard, cap = capacity;
    Staging s(c, BUF_SCRATCH, c->stream);
    const int i_org = s.opt(R > 0 && n_origins != 1, F, 3 * R, origins), i_dirs = s.add(F, 3 * R, dirs), i_dq = s.add(F, R, depth_q),
              i_rgb = s.add(F, 3 * R, premultiplied_rgb), i_op = s.add(F, R, opacity), i_nrm = s.opt(normals, F, 3 * R, normals),
              i_bsum = s.add(4, (R + kSurfaceBlock - 1) / kSurfaceBlock), i_ray_of = s.add(4, R), i_state = s.add(sizeof(PointState), 1, nullptr, nullptr, 0),
              i_xyz = s.add(4, 3 * cap + G, nullptr, xyz_out, 0xFF), i_c = s.add(4, 3 * cap + G, nullptr, rgb_out, 0xFF),
              i_n = s.opt(normals_out, 4, 3 * cap + G, nullptr, normals_out, 0xFF), i_r = s.opt(ray_out, 4, cap + G, nullptr, ray_out, 0xFF),
              i_d = s.opt(depth_out, 4, cap + G, nullptr, depth_out, 0xFF), i_a = s.opt(opacity_out, 4, cap + G, nullptr, opacity_out, 0xFF);
    int rc;
    if ((rc = s.begin())) return rc;
    PointGatherArgs a{};
    a.n_rays = (int)R; a.first_ray = 0; a.origins = s.at(i_org);
    if (R > 0 && n_origins == 1) copy3(a.origin, origins);
    a.dirs = s.at(i_dirs); a.depth_q = s.at(i_dq); a.rgb = s.at(i_rgb); a.opacity = s.at(i_op); a.normals = s.at(i_nrm);
    a.min_opacity = min_opacity; a.capacity = (uint32_t)cap;
    a.bsum = s.at<uint32_t>(i_bsum); a.ray_of = s.at<uint32_t>(i_ray_of); a.state = s.at<PointState>(i_state);
    a.xyz_out = s.at(i_xyz); a.rgb_out = s.at(i_c); a.normals_out = s.at(i_n); a.ray_out = s.at<uint32_t>(i_r); a.depth_out = s.at(i_d);
    a.opacity_out = s.at(i_a);
    HIP_TRY(c, launch_point_gather(a, c->stream));
    HIP_TRY(c, launch_point_total(a.state, nullptr, c->stream));
    PointState hs{};
    HIP_TRY(c, hipMemcpyAsync(&hs, a.state, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    if ((rc = s.finish())) return rc;
    *n_points = hs.running;
    if ((size_t)hs.running > cap) {
        char msg[160];
        snprintf(msg, sizeof msg, "point cloud: %u rays are kept but the capacity is %zu points; the first %zu are written", hs.running, cap, cap);
        return fail(c, NERF_ERR_STATE, msg);
    }
    return NERF_OK;
} NERF_CATCH(c)

} // extern "C"
