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

#include "nerf_internal.h"

using namespace nerfint;

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
    if (dtype == NERF_MLP_F16X2 && !c->net[which].wstream_x2) return fail(c, NERF_ERR_STATE, "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range");
    a.wstream = stream_of(c->net[which], dtype); a.small_params = small_of(c->net[which], dtype); zskip_of(c, c->net[which], a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.dirs_aos = d_dirs; a.sigma_out = d_sigma; a.rgb_out = d_rgb;
    a.nonfinite = nonfinite_of(c, dtype);
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
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, n * 10 * sizeof(float)))) return rc;
    float *d_pts = (float *)c->d_scratch, *d_dirs = d_pts + 3 * n, *d_rgb = d_dirs + 3 * n, *d_sig = d_rgb + 3 * n;
    HIP_TRY(c, hipMemcpyAsync(d_pts, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_dirs, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const bool watch = split_dtype(dtype) && c->d_nonfinite;
    if (watch) HIP_TRY(c, hipMemsetAsync(c->d_nonfinite, 0, sizeof(unsigned int), c->stream));
    if ((rc = forward_device(c, which, dtype, d_pts, d_dirs, n, d_rgb, d_sig, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sigma, d_sig, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    unsigned int bad = 0;
    if (watch) HIP_TRY(c, hipMemcpyAsync(&bad, c->d_nonfinite, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, n * 4 * sizeof(float)))) return rc;
    float *d_pts = (float *)c->d_scratch, *d_sig = d_pts + 3 * n;
    HIP_TRY(c, hipMemcpyAsync(d_pts, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = density_batch_device(c, which, d_pts, n, d_sig, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(sigma, d_sig, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    a.wstream = c->net[which].wstream; a.small_params = c->net[which].small_f32; zskip_of(c, c->net[which], a);
    a.n_points = (int)n_cells; a.sigma_out = d_sigma;
    for (int k = 0; k < 3; ++k) { a.grid_lo[k] = lo[k]; a.grid_step[k] = step[k]; a.grid_n[k] = dims[k]; }
    a.occ_threshold = threshold; a.occ_bits = d_bits;
    HIP_TRY(c, nerf_mlp_launch(a, false, c->n_cus, st));
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
    if (stats && (rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, 8 * sizeof(int)))) return rc;
    int *d_stats = stats ? (int *)c->d_scratch : nullptr;
    if ((rc = density_grid_launch(c, which, lo, step, dims, n_cells, d_sigma_out, threshold, d_occ_bits, d_stats, (hipStream_t)stream))) return rc;
    if (stats) {
        int h[8];
        HIP_TRY(c, hipMemcpyAsync(h, d_stats, sizeof h, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream));
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
    const size_t n_words = occ_bits ? (n_cells + 31) / 32 : 0;
    const size_t bytes = 8 * sizeof(int) + n_words * sizeof(uint32_t) + (sigma_out ? n_cells * sizeof(float) : 0);
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, bytes))) return rc;
    int *d_stats = (int *)c->d_scratch;
    uint32_t *d_bits = occ_bits ? (uint32_t *)(d_stats + 8) : nullptr;
    float *d_sigma = sigma_out ? (float *)(d_stats + 8) + n_words : nullptr;
    if ((rc = density_grid_launch(c, which, lo, step, dims, n_cells, d_sigma, threshold, d_bits, stats ? d_stats : nullptr, c->stream))) return rc;
    int h[8];
    if (sigma_out) HIP_TRY(c, hipMemcpyAsync(sigma_out, d_sigma, n_cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (occ_bits) HIP_TRY(c, hipMemcpyAsync(occ_bits, d_bits, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (stats) HIP_TRY(c, hipMemcpyAsync(h, d_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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

// the dilation and, when asked for, the statistics of its output (through c->d_scratch: 8 ints); arguments already checked
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
    if (stats && (rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, 8 * sizeof(int)))) return rc;
    return dilate_device(c, d_occ_bits, dims, radius, d_occ_out, n_cells, stats ? (int *)c->d_scratch : nullptr, n_occupied, bounds, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_occupancy_dilate(nerf_ctx *c, const uint32_t *occ_bits, const int32_t dims[3], int radius, uint32_t *occ_out, uint64_t *n_occupied,
                          int32_t bounds[6]) try {
    size_t n_cells = 0;
    int rc;
    if ((rc = dilate_check(c, occ_bits, dims, radius, occ_out, &n_cells))) return rc;
    DeviceGuard dg(c->device);
    // staging: [8 ints of statistics][input words][output words]
    const size_t n_words = (n_cells + 31) / 32;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, 8 * sizeof(int) + 2 * n_words * sizeof(uint32_t)))) return rc;
    int *d_stats = (int *)c->d_scratch;
    uint32_t *d_in = (uint32_t *)(d_stats + 8), *d_out = d_in + n_words;
    HIP_TRY(c, hipMemcpyAsync(d_in, occ_bits, n_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = dilate_device(c, d_in, dims, radius, d_out, n_cells, (n_occupied || bounds) ? d_stats : nullptr, n_occupied, bounds, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(occ_out, d_out, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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

// the clip launch on device pointers; with n_hit the block sums go through c->d_clip and the total comes back (one synchronisation)
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
        if ((rc = ensure_bytes(c, &c->d_clip, &c->clip_bytes, (n_blocks + 2) * sizeof(uint32_t)))) return rc;
        d_totals = (uint32_t *)c->d_clip;
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
    // staging (words): occupancy, dirs, origins, [bounds], bounds_out, hit flags
    const size_t R = n_rays, n_words = ((size_t)dims[0] * dims[1] * dims[2] + 31) / 32, n_o = n_origins == 1 ? 1 : R;
    const size_t o_g = 0, o_d = o_g + n_words, o_o = o_d + 3 * R, o_b = o_o + 3 * n_o, o_c = o_b + (bounds ? 2 * R : 0), o_h = o_c + 2 * R,
                 total = o_h + (R + 3) / 4;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * 4))) return rc;
    uint32_t *d = (uint32_t *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_g, occ_bits, n_words * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_d, dirs, 3 * R * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_o, origins, 3 * n_o * 4, hipMemcpyHostToDevice, c->stream));
    if (bounds) HIP_TRY(c, hipMemcpyAsync(d + o_b, bounds, 2 * R * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = clip_device(c, d + o_g, lo, step, dims, (const float *)(d + o_o), n_origins, (const float *)(d + o_d), R, normalize, near_, far_,
                          bounds ? (const float *)(d + o_b) : nullptr, (float *)(d + o_c), (uint8_t *)(d + o_h), n_hit, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(bounds_out, d + o_c, 2 * R * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hit_out, d + o_h, R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    // staging in the scratch, in 256-byte slots: what the caller cannot receive directly, and the inputs / sigma output of the colour launch
    size_t words = 0;
    auto slot = [&](bool wanted, size_t n) { const size_t at = words; if (wanted) words += (n + 63) / 64 * 64; return at; };
    const size_t v_at = slot(host_out && o.vertices, 3 * nv), n_at = slot(host_out && o.normals, 3 * nv), c_at = slot(host_out && o.rgb, 3 * nv),
                 t_at = slot(host_out && o.triangles, 3 * nt), soa_at = slot(o.rgb, 3 * nv), dir_at = slot(o.rgb, 3 * nv), sig_at = slot(o.rgb, nv);
    int rc;
    if (words && (rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, words * sizeof(float)))) return rc;
    float *s = (float *)c->d_scratch;
    float *d_v = !o.vertices ? nullptr : host_out ? s + v_at : o.vertices, *d_n = !o.normals ? nullptr : host_out ? s + n_at : o.normals;
    float *d_c = !o.rgb ? nullptr : host_out ? s + c_at : o.rgb;
    uint32_t *d_t = !o.triangles ? nullptr : host_out ? (uint32_t *)(s + t_at) : o.triangles;
    HIP_TRY(c, launch_mesh_emit(g, w, (uint32_t)nv, d_v, d_n, o.rgb ? s + soa_at : nullptr, o.rgb ? s + dir_at : nullptr, (uint32_t)nt, d_t, st));
    if (o.rgb && (rc = forward_device(c, colour_net, NERF_MLP_F32, s + soa_at, s + dir_at, nv, d_c, s + sig_at, st))) return rc;
    if (host_out) {
        if (o.vertices) HIP_TRY(c, hipMemcpyAsync(o.vertices, d_v, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, st));
        if (o.normals) HIP_TRY(c, hipMemcpyAsync(o.normals, d_n, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, st));
        if (o.rgb) HIP_TRY(c, hipMemcpyAsync(o.rgb, d_c, 3 * nv * sizeof(float), hipMemcpyDeviceToHost, st));
        if (o.triangles && nt) HIP_TRY(c, hipMemcpyAsync(o.triangles, d_t, 3 * nt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    return NERF_OK;
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
    if ((rc = ensure_bytes(c, &c->d_comp, &c->comp_bytes, comp_workspace_bytes(n)))) return rc;
    const MeshWorkspace mw = mesh_workspace_carve(c->d_mesh, n);
    *out = comp_workspace_carve(c->d_comp, n, mw.vbase, mw.tbase);
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
    if ((rc = ensure_bytes(c, &c->d_mesh, &c->mesh_bytes, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace w = mesh_workspace_carve(c->d_mesh, n);
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
    if ((rc = ensure_bytes(c, &c->d_mesh, &c->mesh_bytes, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace mw = mesh_workspace_carve(c->d_mesh, n);
    HIP_TRY(c, hipMemcpyAsync(mw.sigma, sigma, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return lattice_components(c, mw.sigma, dims, iso, n, labels_out, true, (nerf_component *)table, cap_table, n_components, c->stream);
} NERF_CATCH(c)

int nerf_lattice_components_device(nerf_ctx *c, const float *d_sigma, const int32_t dims[3], float iso, uint32_t *d_labels_out, void *table, size_t cap_table,
                                   uint64_t *n_components, void *stream) try {
    size_t n = 0;
    int rc;
    if ((rc = components_check(c, d_sigma, dims, iso, table, cap_table, n_components, &n))) return rc;
    DeviceGuard dg(c->device);
    if ((rc = ensure_bytes(c, &c->d_mesh, &c->mesh_bytes, mesh_workspace_bytes(n)))) return rc;
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
    if ((rc = ensure_bytes(c, &c->d_mesh, &c->mesh_bytes, mesh_workspace_bytes(n)))) return rc;
    const MeshWorkspace w = mesh_workspace_carve(c->d_mesh, n);
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
    if ((rc = ensure_bytes(c, &c->d_stencil, &c->stencil_bytes, 6 * chunk * 4 * sizeof(float)))) return rc;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        float *d_spts = (float *)c->d_stencil, *d_ssig = d_spts + 18 * m;
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
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, n * 6 * sizeof(float)))) return rc;
    float *d_pts = (float *)c->d_scratch, *d_grad = d_pts + 3 * n;
    HIP_TRY(c, hipMemcpyAsync(d_pts, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = density_gradient_device(c, which, d_pts, n, h, d_grad, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(grad, d_grad, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    const size_t bytes = (size_t)g.n_rays * 3 * sizeof(float);
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, bytes))) return rc;
    HIP_TRY(c, launch_ray_dirs(g, (float *)c->d_scratch, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scratch, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
} NERF_CATCH(c)

int nerf_stage_stratified(nerf_ctx *c, const nerf_camera *cam, int x0, int y0, int w, int h, int count, uint64_t seed, float *out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (count <= 0) return NERF_OK; // src/lib.rs:235-237
    DeviceGuard dg(c->device);
    RayGenArgs g; int rc;
    if ((rc = stage_rect(c, cam, x0, y0, w, h, g))) return rc;
    const size_t bytes = (size_t)g.n_rays * count * sizeof(float);
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, bytes))) return rc;
    HIP_TRY(c, launch_stratified(g, count, cam->near_, cam->far_, seed, (float *)c->d_scratch, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_scratch, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    // layout in scratch (floats): tc, sc, u, w, cdf, tnew, tfine, pix
    const size_t o_tc = 0, o_sc = o_tc + R * nc, o_u = o_sc + R * nc, o_w = o_u + R * nf, o_cdf = o_w + R * nc,
                 o_tn = o_cdf + R * (nc - 1), o_tf = o_tn + R * nf, o_px = o_tf + R * M, o_fl = o_px + R, total = o_fl + (R + 3) / 4;
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * sizeof(float)))) return rc;
    float *d = (float *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_tc, t_coarse, R * nc * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_sc, sigma_coarse, R * nc * 4, hipMemcpyHostToDevice, c->stream));
    if (u) HIP_TRY(c, hipMemcpyAsync(d + o_u, u, R * nf * 4, hipMemcpyHostToDevice, c->stream));
    if (pixel_index) HIP_TRY(c, hipMemcpyAsync(d + o_px, pixel_index, R * 4, hipMemcpyHostToDevice, c->stream));
    ResampleArgs ra{};
    ra.n_rays = (int)R; ra.nc = nc; ra.nf = nf; ra.far_ = far_;
    ra.seed_lo = (uint32_t)seed; ra.seed_hi = (uint32_t)(seed >> 32);
    ra.t_coarse = d + o_tc; ra.sigma_coarse = d + o_sc; ra.t_fine = d + o_tf;
    ra.pixel_index = pixel_index ? (const uint32_t *)(d + o_px) : nullptr;
    ra.u_in = u ? d + o_u : nullptr;
    ra.w_out = d + o_w; ra.cdf_out = d + o_cdf; ra.t_new_out = d + o_tn;
    ra.g.rw = 1; ra.g.rnx = 1; // unused when pixel_index/u are given
    if (flags_out) { ra.flag_tau = tau; ra.flag_out = (unsigned char *)(d + o_fl); }
    HIP_TRY(c, launch_resample(ra, c->stream));
    if (flags_out) HIP_TRY(c, hipMemcpyAsync(flags_out, d + o_fl, R, hipMemcpyDeviceToHost, c->stream));
    if (w_out) HIP_TRY(c, hipMemcpyAsync(w_out, d + o_w, R * nc * 4, hipMemcpyDeviceToHost, c->stream));
    if (cdf_out) HIP_TRY(c, hipMemcpyAsync(cdf_out, d + o_cdf, R * (nc - 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (t_new_out) HIP_TRY(c, hipMemcpyAsync(t_new_out, d + o_tn, R * nf * 4, hipMemcpyDeviceToHost, c->stream));
    if (t_fine_out) HIP_TRY(c, hipMemcpyAsync(t_fine_out, d + o_tf, R * M * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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

int nerf_stage_depth_order(nerf_ctx *c, int rows, int rays_per_row, int samples_per_ray, const float *t, uint32_t *table_out) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!t || !table_out) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (rows <= 0 || rays_per_row <= 0 || samples_per_ray <= 0 || (long long)rows * rays_per_row * samples_per_ray > 0x3fffffff)
        return fail(c, NERF_ERR_INVALID, "rows, rays_per_row and samples_per_ray must be > 0 and within one pass");
    const int n = rows * rays_per_row * samples_per_ray;
    const nerfmlp::DepthOrder d = nerfmlp::depth_order_of(n, samples_per_ray, rays_per_row, true, true); // as the full launch of an image pass of this shape
    if (d.tiles == 0) return fail(c, NERF_ERR_INVALID, "this window is not depth-ordered: rays_per_row % 8 == 0, rows >= 4, samples_per_ray % 32 == 0 and <= 512");
    DeviceGuard dg(c->device);
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, ((size_t)n + d.points) * 4))) return rc;
    float *d_t = (float *)c->d_scratch;
    unsigned int *d_table = (unsigned int *)(d_t + n);
    HIP_TRY(c, hipMemcpyAsync(d_t, t, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    DepthOrderArgs q{};
    q.t = d_t; q.rw = rays_per_row; q.spr = samples_per_ray; q.blocks_x = d.blocks_x; q.blocks = d.blocks; q.table = d_table;
    HIP_TRY(c, launch_depth_order(q, c->stream));
    HIP_TRY(c, hipMemcpyAsync(table_out, d_table, (size_t)d.points * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    const size_t o_t = 0, o_s = o_t + R * N, o_c = o_s + R * N, o_w = o_c + 3 * R * N, o_o = o_w + R * N, total = o_o + 3 * R;
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * sizeof(float)))) return rc;
    float *d = (float *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_t, t, R * N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_s, sigma, R * N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_c, rgb, 3 * R * N * 4, hipMemcpyHostToDevice, c->stream));
    CompositeArgs ca{};
    ca.n_rays = (int)R; ca.n = n; ca.far_ = far_; ca.t = d + o_t; ca.sigma = d + o_s; ca.rgb = d + o_c; ca.out = d + o_o; ca.w_out = d + o_w;
    HIP_TRY(c, launch_composite(ca, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rgb_out, d + o_o, 3 * R * 4, hipMemcpyDeviceToHost, c->stream));
    if (w_out) HIP_TRY(c, hipMemcpyAsync(w_out, d + o_w, R * N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    // scratch (floats): t, sigma, rgb, per-ray colour, per-ray opacity, packed words
    const size_t o_t = 0, o_s = o_t + R * N, o_c = o_s + R * N, o_o = o_c + 3 * R * N, o_a = o_o + 3 * R, o_p = o_a + R, total = o_p + R;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * sizeof(float)))) return rc;
    float *d = (float *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_t, t, R * N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_s, sigma, R * N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_c, rgb, 3 * R * N * 4, hipMemcpyHostToDevice, c->stream));
    CompositeArgs ca{};
    ca.n_rays = (int)R; ca.n = n; ca.far_ = far_; ca.t = d + o_t; ca.sigma = d + o_s; ca.rgb = d + o_c; ca.out = d + o_o;
    ca.opacity = alpha_mode == NERF_ALPHA_OPAQUE ? nullptr : d + o_a;
    if (bg) { ca.use_bg = 1; ca.bg[0] = bg[0]; ca.bg[1] = bg[1]; ca.bg[2] = bg[2]; }
    HIP_TRY(c, launch_composite(ca, c->stream));
    HIP_TRY(c, launch_pack_rgba8(ca.out, ca.opacity, (uint32_t *)(d + o_p), R, alpha_mode, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rgba_out, d + o_p, R * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    // scratch (words): pre, t, jstar, three counters (+ 1), guarded list, guarded aux
    const size_t o_pre = 0, o_t = o_pre + N, o_j = o_t + N, o_cnt = o_j + n_rays, o_list = o_cnt + 4, o_aux = o_list + n_list, total = o_aux + n_aux;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * 4))) return rc;
    uint32_t *d = (uint32_t *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_pre, pre, N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_t, t, N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_j, 0xFF, n_rays * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_cnt, 0, 4 * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_list, 0xFF, (n_list + n_aux) * 4, c->stream));
    CertPlanArgs q{};
    q.pre = (float *)(d + o_pre); q.t = (const float *)(d + o_t); q.n_rays = (int)n_rays; q.spr = spr; q.far_ = far_;
    q.margin = margin; q.depth_limit = depth_limit; q.audit_mask = audit_mask; q.audit_mask_near = audit_mask_near; q.audit_salt = audit_salt;
    q.list = d + o_list + kStageGuard; q.count = d + o_cnt; q.capacity = list_capacity; q.jstar = (int *)(d + o_j);
    if (back_part) { q.count_back = d + o_cnt + 1; q.zero_threshold = zero_threshold; }
    q.aux = d + o_aux + kStageGuard; q.aux_count = d + o_cnt + 2; q.aux_capacity = aux_capacity;
    HIP_TRY(c, launch_cert_plan(q, c->stream));
    HIP_TRY(c, hipMemcpyAsync(pre, d + o_pre, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(jstar_out, d + o_j, n_rays * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts_out, d + o_cnt, 3 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(list_out, d + o_list, n_list * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(aux_out, d + o_aux, n_aux * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    // scratch (words): sigma, t, jstar, {count, fall-back rays}, guarded list
    const size_t o_s = 0, o_t = o_s + N, o_j = o_t + N, o_cnt = o_j + n_rays, o_list = o_cnt + 2, total = o_list + n_list;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * 4))) return rc;
    uint32_t *d = (uint32_t *)c->d_scratch;
    const uint32_t cnt[2] = {*count, *fallback_rays};
    HIP_TRY(c, hipMemcpyAsync(d + o_s, sigma, N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_t, t, N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_j, jstar, n_rays * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_list, 0xFF, n_list * 4, c->stream));
    CertVerifyArgs v{};
    v.t = (const float *)(d + o_t); v.sigma = (float *)(d + o_s); v.n_rays = (int)n_rays; v.spr = spr; v.far_ = far_; v.jstar = (const int *)(d + o_j);
    v.list = d + o_list + kStageGuard; v.count = d + o_cnt; v.capacity = list_capacity; v.fallback_rays = d + o_cnt + 1;
    HIP_TRY(c, launch_cert_verify(v, c->stream));
    uint32_t back[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(sigma, d + o_s, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(back, d + o_cnt, sizeof back, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(list_out, d + o_list, n_list * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *count = back[0]; *fallback_rays = back[1];
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
    // scratch (words): sigma, the records, the count, the four audit words
    const size_t o_s = 0, o_a = o_s + n_sigma, o_cnt = o_a + 2 * n_rec, o_w = o_cnt + 1, total = o_w + 4;
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * 4))) return rc;
    uint32_t *d = (uint32_t *)c->d_scratch;
    if (n_sigma) HIP_TRY(c, hipMemcpyAsync(d + o_s, sigma, n_sigma * 4, hipMemcpyHostToDevice, c->stream));
    if (n_rec) HIP_TRY(c, hipMemcpyAsync(d + o_a, aux, 2 * n_rec * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_cnt, &aux_count, 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_w, audit, 4 * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_cert_audit(d + o_a, d + o_cnt, aux_capacity, (float *)(d + o_s), d + o_w, c->n_cus, c->stream));
    if (n_sigma) HIP_TRY(c, hipMemcpyAsync(sigma, d + o_s, n_sigma * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(audit, d + o_w, 4 * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    if (f16 && !net.wstream_f16v2) return fail(c, NERF_ERR_STATE, "the f16 pre-filter is unavailable for this network: a weight exceeds the f16 range");
    *nonfinite_tiles = 0;
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    const size_t N = n_rays * (size_t)spr;
    // scratch (words): directions, t, pre-activations, {ray queue, non-finite tiles, samples evaluated (64 bits)}, [origins]
    const size_t o_d = 0, o_t = o_d + 3 * n_rays, o_p = o_t + N, o_cnt = (o_p + N + 1) & ~(size_t)1, o_o = o_cnt + 4, total = o_o + (origins ? 3 * n_rays : 0);
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, total * 4))) return rc;
    uint32_t *d = (uint32_t *)c->d_scratch;
    HIP_TRY(c, hipMemcpyAsync(d + o_d, dirs, 3 * n_rays * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d + o_t, t, N * 4, hipMemcpyHostToDevice, c->stream));
    if (origins) HIP_TRY(c, hipMemcpyAsync(d + o_o, origins, 3 * n_rays * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d + o_p, 0xFF, N * 4, c->stream)); // NaN = "not evaluated", as cert_pass fills it
    HIP_TRY(c, hipMemsetAsync(d + o_cnt, 0, 4 * 4, c->stream));
    SeqArgs q{};
    q.wstream = f16 ? (const float *)net.wstream_f16v2 : stream_of(net, NERF_MLP_BF16); q.small_params = net.small;
    q.n_rays = (int)n_rays; q.samples_per_ray = spr; q.ray_dirs = (const float *)(d + o_d); q.t = (const float *)(d + o_t); q.far_ = far_;
    if (origins) q.ray_origins = (const float *)(d + o_o);
    else copy3(q.origin, origin);
    q.sigma_out = (float *)(d + o_p);
    q.ray_counter = d + o_cnt; q.nonfinite = d + o_cnt + 1; q.stats = (unsigned long long *)(d + o_cnt + 2);
    q.prefilter = 1; q.prefilter_cut_T = cut_T;
    HIP_TRY(c, f16 ? nerf_trunk_seq_f16v2_launch(q, c->n_cus, c->stream) : nerf_trunk_seq_bf16_launch(q, false, c->n_cus, c->stream));
    HIP_TRY(c, hipMemcpyAsync(pre_out, d + o_p, N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(nonfinite_tiles, d + o_cnt + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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

} // extern "C"
