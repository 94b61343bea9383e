// nerf_render.cpp -- the renders: the pass pipeline that image renders and ray batches share, their drivers, certify_zero's retry loop, and
// the nerf_render_* entry points (include/nerf_mi355x.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "host_util.h"
#include "mlp_kernel.h"
#include "mlp_layout.h"
#include "normal_kernels.h"
#include "ray_batch_kernels.h"
#include "ray_clip_core.h"
#include "ray_clip_kernels.h"
#include "sampling_kernels.h"
#include "surface_kernels.h"

using namespace nerfhost;

#include "nerf_internal.h"

using namespace nerfint;

namespace nerfint {

RayGenArgs make_raygen(const nerf_camera &cam, int s) {
    RayGenArgs g{};
    g.rnx = cam.nx * s; g.rny = cam.ny * s;
    g.half = 0.5f; g.normalize = 1;
    camera_basis(cam, g.r, g.u, g.f, &g.sx, &g.sy);
    return g;
}

int check_camera(nerf_ctx *c, const nerf_camera *cam) {
    if (!cam) return fail(c, NERF_ERR_INVALID, "camera is NULL");
    if (cam->nx <= 0 || cam->ny <= 0) return fail(c, NERF_ERR_INVALID, "width and height must be greater than zero"); // src/lib.rs:705-709
    return NERF_OK;
}

// what the three alpha modes ask of the compositing kernel: the background it adds (NULL: the reference's white) and whether the pack
// kernel needs the opacity plane
int check_rgba8(nerf_ctx *c, const float *background, int alpha_mode, const void *out, const float **bg_composite) {
    static const float kBlack[3] = {0.0f, 0.0f, 0.0f};
    if (alpha_mode != NERF_ALPHA_OPAQUE && alpha_mode != NERF_ALPHA_PREMULTIPLIED && alpha_mode != NERF_ALPHA_STRAIGHT)
        return fail(c, NERF_ERR_INVALID, "alpha_mode must be NERF_ALPHA_OPAQUE, NERF_ALPHA_PREMULTIPLIED or NERF_ALPHA_STRAIGHT");
    if (background && !(std::isfinite(background[0]) && std::isfinite(background[1]) && std::isfinite(background[2])))
        return fail(c, NERF_ERR_INVALID, "background components must be finite");
    if (!out) return fail(c, NERF_ERR_INVALID, "output pointer is NULL");
    *bg_composite = alpha_mode == NERF_ALPHA_OPAQUE ? background : kBlack; // premultiplied / straight: C + 0 * (1 - A) = C
    return NERF_OK;
}

} // namespace nerfint

namespace {

// What the fourteen nerf_render_rays* entry points receive.  A host form stages its request (render_rays_entry) into one whose pointers are
// device pointers and hands that to the device form.
struct RayRequest {
    const float *origins; size_t n_origins; // n_origins x 3; n_origins is 1 (one origin for every ray) or n_rays
    const float *dirs; size_t n_rays;       // n_rays x 3
    int normalize;
    float near_, far_;
    const float *bounds;                    // n_rays x 2, or NULL
    const uint32_t *rng_index;              // n_rays, or NULL
    const nerf_render_opts *opts;
    const float *background;                // 3 floats on the host, or NULL
    float *rgb, *depth, *opacity;           // per ray; depth and opacity may be NULL
    bool want_normals; float h; float *normals; // nerf_render_rays_normals*
    bool clipped;                           // nerf_render_rays_clipped*: the grid (lo, step, dims on the host), the flags and the hit count
    const uint32_t *occ_bits; const float *lo, *step; const int32_t *dims; uint8_t *hit; uint64_t *n_hit;
    bool certified;                         // nerf_render_rays*_certified*
    bool want_quantiles; int n_q; const float *quantiles; float *depth_q; // nerf_render_rays_quantiles*: n_q targets on the HOST, n_q x n_rays planes
    // nerf_render_rays_points*: one target, the threshold, the normals' step h above (0: none), the outputs (capacity points each) and the count
    bool points; float quantile, min_opacity; size_t capacity;
    float *p_xyz, *p_rgb, *p_normals, *p_depth, *p_opacity; uint32_t *p_ray; size_t *n_points; uint32_t *d_n_points;
    hipStream_t st;
    nerf_stats *stats;
    const float *h_origin;                  // device requests with n_origins == 1: the shared origin on the HOST once it is known
};

// The pass workspace of a normals render in BUF_NORMAL (StageLayout: every part 256-byte aligned).
struct NormalWorkspace {
    float *w = nullptr; uint32_t *list = nullptr, *count = nullptr, *base = nullptr, *bsum = nullptr, *totals = nullptr;
    size_t bytes = 0;
    NormalWorkspace() = default;
    NormalWorkspace(void *p, size_t rays, size_t samples) { // p == NULL: only `bytes`
        StageLayout l;
        const int i_w = l.add(4, samples), i_list = l.add(4, samples), i_count = l.add(4, rays), i_base = l.add(4, rays),
                  i_bsum = l.add(4, (rays + kNormalBlock - 1) / kNormalBlock), i_totals = l.add(4, 2);
        bytes = l.total;
        if (!p) return;
        w = l.at<float>(p, i_w); list = l.at<uint32_t>(p, i_list); count = l.at<uint32_t>(p, i_count); base = l.at<uint32_t>(p, i_base);
        bsum = l.at<uint32_t>(p, i_bsum); totals = l.at<uint32_t>(p, i_totals);
    }
};

// The workspace of a quantile or points render in BUF_SURFACE (StageLayout: every part 256-byte aligned): per pass the weights (unless a normals
// workspace holds them: samples == 0) and, for a points render, per ray of the BATCH what the compaction reads -- the compositing kernel's
// outputs land there pass by pass -- with the pass's kept-ray list, its block sums and the running count.
struct SurfaceWorkspace {
    float *w = nullptr, *rgb = nullptr, *opacity = nullptr, *depth_q = nullptr, *normals = nullptr;
    uint32_t *ray_of = nullptr, *bsum = nullptr; PointState *state = nullptr;
    size_t bytes = 0;
    SurfaceWorkspace() = default;
    SurfaceWorkspace(void *p, size_t samples, size_t pass_rays, size_t batch_rays, bool with_normals) { // p == NULL: only `bytes`; batch_rays == 0: no points
        StageLayout l;
        const bool pts = batch_rays > 0;
        const int i_w = l.opt(samples > 0, 4, samples), i_rgb = l.opt(pts, 12, batch_rays), i_op = l.opt(pts, 4, batch_rays), i_dq = l.opt(pts, 4, batch_rays),
                  i_nrm = l.opt(pts && with_normals, 12, batch_rays), i_ray = l.opt(pts, 4, pass_rays),
                  i_bsum = l.opt(pts, 4, (pass_rays + kSurfaceBlock - 1) / kSurfaceBlock), i_state = l.opt(pts, sizeof(PointState), 1);
        bytes = l.total;
        if (!p) return;
        w = l.at<float>(p, i_w); rgb = l.at<float>(p, i_rgb); opacity = l.at<float>(p, i_op); depth_q = l.at<float>(p, i_dq); normals = l.at<float>(p, i_nrm);
        ray_of = l.at<uint32_t>(p, i_ray); bsum = l.at<uint32_t>(p, i_bsum); state = l.at<PointState>(p, i_state);
    }
};

// The workspace of a clipped render (nerf_render_rays_clipped) in BUF_CLIP for a batch of n rays (StageLayout: every part 256-byte aligned):
// the clip's outputs, the block sums, and the compacted batch with its outputs (sized for n hits, so that the hit count never reallocates).
struct ClipWorkspace {
    uint32_t *totals = nullptr, *bsum = nullptr, *ray_of = nullptr, *rng_c = nullptr;
    float *clip_bounds = nullptr, *dirs_c = nullptr, *origins_c = nullptr, *bounds_c = nullptr, *rgb_c = nullptr, *depth_c = nullptr, *opacity_c = nullptr;
    uint8_t *hit = nullptr;
    size_t bytes = 0;
    ClipWorkspace(void *p, size_t n, bool per_ray_origins) { // p == NULL: only `bytes`
        StageLayout l;
        const int i_totals = l.add(4, 2), i_bsum = l.add(4, (n + kClipBlock - 1) / kClipBlock), i_hit = l.add(1, n), i_cb = l.add(8, n),
                  i_ray = l.add(4, n), i_rng = l.add(4, n), i_dirs = l.add(12, n), i_org = l.add(12, per_ray_origins ? n : 0), i_bounds = l.add(8, n),
                  i_rgb = l.add(12, n), i_depth = l.add(4, n), i_opacity = l.add(4, n);
        bytes = l.total;
        if (!p) return;
        totals = l.at<uint32_t>(p, i_totals); bsum = l.at<uint32_t>(p, i_bsum); hit = l.at<uint8_t>(p, i_hit); clip_bounds = l.at<float>(p, i_cb);
        ray_of = l.at<uint32_t>(p, i_ray); rng_c = l.at<uint32_t>(p, i_rng); dirs_c = l.at<float>(p, i_dirs); origins_c = l.at<float>(p, i_org);
        bounds_c = l.at<float>(p, i_bounds); rgb_c = l.at<float>(p, i_rgb); depth_c = l.at<float>(p, i_depth); opacity_c = l.at<float>(p, i_opacity);
    }
};

// ---- the pass pipeline ------------------------------------------------------------------------------------------------------------------
// Host counterpart of render_image / render_block (reference src/lib.rs:353-565): where the reference cuts the frame in 8x8 blocks for rayon
// workers, a render here is cut in "passes" of at most max_rays_per_pass rays (all resident in HBM), and per pass
//     rays + coarse t -> coarse MLP (sigma) -> [composite, if coarse_only] -> resample/sort -> fine MLP -> composite
// run as launches on one stream with no host round trip (a normals render has one per pass, normals_pass).  Image renders (render_once) and
// ray batches (render_rays_device) validate their own arguments, fill a RenderJob and run the same loop, render_passes; they differ in
// where a pass's rays come from (prepare_rays) and in how a network is evaluated over a pass's samples (eval_net).

// What a render does, as plain data: filled by the two drivers after validation, read-only afterwards.
struct RenderJob {
    // the sample plan (plan_job)
    int nc, nf, M;           // coarse samples, fine samples added by the resampler (0: none), samples of the fine pass
    int dtype, dtype_coarse; // arithmetic of the colour-producing pass / of the sampling pass
    bool coarse_only;
    uint64_t seed;
    float near_, far_;       // the shared bounds ...
    float *d_far;            // ... or, for a batch with per-ray bounds, the far of each ray of the pass under way (k_batch_prepare writes it)
    float far_cert;          // certify_zero: the far the certify kernels are given -- far_, or below every t for per-ray bounds (cert_pass)
    const float *background; // 3 floats, or NULL = the reference's white
    // outputs, per ray: the pass that starts at ray r0 writes out + 3 r0, depth + r0, opacity + r0 (r0 = row x RW of an image)
    float *out, *depth, *opacity;
    size_t n_rays, pass_rays; // all rays, rays of a full pass
    EvKind kind_colour;       // of the colour-producing launch: EV_IMAGE_COLOUR (-> c->dominant) or EV_BATCH_COLOUR
    const char *what;         // "frame" / "batch", for the non-finite error
    hipStream_t st;
    // modes (skip_empty, skip_dead, hybrid_sampling: images only, ray batches refuse them)
    int skip_empty;
    bool seq, hybrid, certify; // skip_dead, hybrid_sampling with something to resample, certify_zero (batches: nerf_render_rays_certified)
    size_t cert_cap, aux_cap;  // certify_zero: capacity of the sample list and of the audit records
    unsigned long long *clock_out; // NERF_DEBUG_CLOCK: where the fine launch leaves its clocks
    // the ray source: a camera window (g: everything but the pass's own n_rays and first row) or the caller's rays
    const RayRequest *batch;   // device pointers
    RayGenArgs g;
    float origin[3];           // the shared origin (batches with per-ray origins: unused)
    float *d_pts, *d_daos;     // per-ray origins, uncertified: the points and per-sample directions of one launch (k_batch_points)
    // normals (batches only): per-ray output, central-difference step, samples per ray the final compositing integrates, pass workspace
    float *normals; float h; int n_comp; NormalWorkspace nw;
    // quantile depths (batches only): n_q targets, the planes (plane k of the batch at depth_q + k * depth_q_stride) and the weights the walk
    // reads -- the normals workspace's when the render also makes normals, else the surface workspace's; points: the compaction's pass
    // template (outputs, thresholds, workspace) or points == false
    int n_q; float quant[kSurfaceMaxQuantiles]; float *depth_q; size_t depth_q_stride; float *w_surface;
    bool points; PointGatherArgs pg;
};

struct Pass {
    uint32_t index;
    size_t r0;             // first ray
    int n_rays;
    RayGenArgs g;          // what the resampler derives its Philox index from (unless rng is given): the image rectangle of the pass, or
                           // for a batch the ray's number in it -- a one-row rectangle that starts at column r0
    const uint32_t *rng;   // the caller's rng_index for the pass's rays, or NULL
    const float *origins;  // per-ray origins of the pass, or NULL
};

bool watches_range(const nerf_ctx *c, const RenderJob &j) { return c->buf[BUF_NONFINITE].p && (arith_of(j.dtype).counts_range || arith_of(j.dtype_coarse).counts_range); }

// sample_importance returns nothing for count == 0 or < 3 coarse samples (src/lib.rs:295-297): the fine net then runs on the coarse samples only
int fine_samples(const nerf_render_opts *o) { return (o->coarse_only || o->n_fine == 0 || o->n_coarse < 3) ? 0 : o->n_fine; }

// The sample plan's checks, shared by image renders and ray batches; each caller runs the three parts where its own order of refusals has them.
enum PlanPart { PLAN_COUNTS, PLAN_NETWORKS, PLAN_LIMITS };
int check_sample_plan(nerf_ctx *c, const nerf_render_opts *o, PlanPart part) {
    if (part == PLAN_COUNTS) {
        if (o->n_coarse <= 0) return fail(c, NERF_ERR_INVALID, "coarse samples per ray must be greater than 0"); // src/lib.rs:483-486
        if (o->n_fine < 0) return fail(c, NERF_ERR_INVALID, "fine samples per ray must be >= 0");
        if (!valid_dtype(o->mlp_dtype)) return fail(c, NERF_ERR_INVALID, "mlp_dtype must be NERF_MLP_F32, NERF_MLP_BF16, NERF_MLP_BF16X3 or NERF_MLP_F16X2");
    } else if (part == PLAN_NETWORKS) {
        if (!c->net[NERF_NET_COARSE].loaded) return fail(c, NERF_ERR_STATE, "coarse network not loaded");
        if (!o->coarse_only && !c->net[NERF_NET_FINE].loaded) return fail(c, NERF_ERR_STATE, "fine network not loaded");
        if (!available(c->net[o->coarse_only ? NERF_NET_COARSE : NERF_NET_FINE], o->mlp_dtype) ||
            (o->hybrid_sampling && !available(c->net[NERF_NET_COARSE], o->mlp_dtype))) // of a loaded network only NERF_MLP_F16X2 can be missing
            return fail(c, NERF_ERR_STATE, "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range");
    } else {
        const int nc = o->n_coarse, nf = fine_samples(o);
        if ((long long)nc + nf > 0x3fffffff || composite_lds_bytes(nc + nf) > 160 * 1024 || (nf > 0 && resample_lds_bytes(nc, nf) > 160 * 1024))
            return fail(c, NERF_ERR_INVALID, "too many samples per ray for the sampling / compositing kernels (one ray per wave in LDS)");
    }
    return NERF_OK;
}

// bf16x3 / f16x2: the sampling pass (coarse sigma -> CDF -> fine sample positions) stays on the exact-f32 MFMA kernel, so the fine
// samples sit where the f32 path puts them bit for bit (a 1e-5 density difference can move a CDF entry across a fixed
// uniform draw and relocate a sample -- a discontinuity, not an accuracy problem); only the colour-producing pass runs in
// the three-way split arithmetic.
// hybrid_sampling: the sampling pass itself runs in a split arithmetic (the render's own, or -- for an f32 render -- f16x2 where
// the network fits the f16 range, else bf16x3) and only the ill-conditioned rays are redone in f32.
void plan_job(const nerf_ctx *c, const nerf_render_opts *o, RenderJob &j) {
    j.nc = o->n_coarse; j.nf = fine_samples(o); j.M = j.nc + j.nf;
    j.coarse_only = o->coarse_only != 0;
    j.seed = o->seed;
    j.dtype = o->mlp_dtype;
    j.dtype_coarse = o->hybrid_sampling ? (split_dtype(j.dtype) ? j.dtype : available(c->net[NERF_NET_COARSE], NERF_MLP_F16X2) ? NERF_MLP_F16X2 : NERF_MLP_BF16X3)
                                        : (split_dtype(j.dtype) && !o->coarse_only) ? NERF_MLP_F32 : j.dtype;
}

// a pass must keep rays * samples within int32 (kernel indices) as well as within the configured budget
size_t pass_capacity(const nerf_ctx *c, int M) { return std::max<size_t>(1, std::min<size_t>(c->max_rays_per_pass, (size_t)0x3fffffff / (size_t)M)); }

// step 1: c->dev(BUF_DIRS) and the coarse t in c->dev(BUF_TC) for the rays of pass p; fills what the later steps need to know about those rays
int prepare_rays(nerf_ctx *c, const RenderJob &j, Pass &p) {
    if (!j.batch) {
        p.g = j.g; p.g.n_rays = p.n_rays; p.g.ry0 += (int)(p.r0 / (size_t)j.g.rw);
        return timed(c, j.st, EV_OTHER, 0, [&]() -> int {
            HIP_TRY(c, launch_ray_dirs(p.g, c->dev(BUF_DIRS), j.st));
            HIP_TRY(c, launch_stratified(p.g, j.nc, j.near_, j.far_, j.seed, c->dev(BUF_TC), j.st));
            return NERF_OK;
        });
    }
    const RayRequest &b = *j.batch;
    const size_t r0 = p.r0;
    p.rng = b.rng_index ? b.rng_index + r0 : nullptr;
    p.origins = b.n_origins != 1 ? b.origins + 3 * r0 : nullptr;
    p.g.n_rays = p.n_rays; p.g.rx0 = (int)r0; p.g.ry0 = 0; p.g.rw = p.n_rays; p.g.rnx = p.n_rays; p.g.rny = 1;
    BatchPrepareArgs q{};
    q.n_rays = p.n_rays; q.first_ray = (uint32_t)r0; q.dirs = b.dirs + 3 * r0; q.normalize = b.normalize ? 1 : 0;
    q.bounds = b.bounds ? b.bounds + 2 * r0 : nullptr; q.rng_index = p.rng;
    q.near_ = b.near_; q.far_ = b.far_; q.count = j.nc; q.seed_lo = (uint32_t)j.seed; q.seed_hi = (uint32_t)(j.seed >> 32);
    q.dirs_out = c->dev(BUF_DIRS); q.t_out = c->dev(BUF_TC); q.far_out = j.d_far;
    return timed(c, j.st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_batch_prepare(q, j.st)); return NERF_OK; });
}

// what every ray-sequential launch of a pass has in common: one network's trunk over the pass's rays from the shared origin
SeqArgs seq_args(const nerf_ctx *c, const RenderJob &j, const Pass &p, int spr, const float *t, float *sigma_out) {
    SeqArgs q{};
    q.n_rays = p.n_rays; q.samples_per_ray = spr;
    q.ray_dirs = c->dev(BUF_DIRS); q.t = t; q.far_ = j.far_;
    copy3(q.origin, j.origin);
    q.sigma_out = sigma_out;
    return q;
}

// skip_dead: one network over the rays of the pass as ray-sequential trunk [+ colour head on the live samples]
int seq_pass(nerf_ctx *c, const RenderJob &j, const Pass &p, const DevNet &net, int dt, int spr, const float *t_in, float *sigma_out, float *rgb_out,
             int slot, EvKind kind_trunk) {
    const hipStream_t st = j.st;
    SeqCounters *ctr = c->dev<SeqCounters>(BUF_SEQ) + slot;
    HIP_TRY(c, hipMemsetAsync(sigma_out, 0, (size_t)p.n_rays * spr * sizeof(float), st)); // samples behind the cut stay 0
    if (rgb_out) HIP_TRY(c, hipMemsetAsync(rgb_out, 0, (size_t)p.n_rays * spr * 3 * sizeof(float), st)); // weight-0 samples: 0 * 0
    const Arith &ar = arith_of(dt);
    SeqArgs q = seq_args(c, j, p, spr, t_in, sigma_out);
    fill_net(c, net, dt, q);
    q.ray_counter = &ctr->ray_head; q.live_count = &ctr->live_count; q.h8 = c->dev(BUF_H8); q.slot_point = c->dev<unsigned int>(BUF_SLOT_POINT);
    q.rgb_out = rgb_out; // f32: colour passes inside the trunk launch
    q.stats = &ctr->evaluated;
    int rc = timed(c, st, kind_trunk, (uint64_t)p.n_rays * spr, [&]() -> int { HIP_TRY(c, ar.trunk(q, rgb_out != nullptr, c->n_cus, st)); return NERF_OK; });
    if (rc || !rgb_out || !ar.colour) return rc;
    ColourArgs k{};
    k.wstream = q.wstream; k.small_params = q.small_params; k.live_count = &ctr->live_count; k.h8 = c->dev(BUF_H8); k.slot_point = c->dev<unsigned int>(BUF_SLOT_POINT);
    k.ray_dirs = c->dev(BUF_DIRS); k.samples_per_ray = spr; k.rgb_out = rgb_out; k.nonfinite = q.nonfinite;
    return timed(c, st, EV_COLOUR_SIDE, 0, [&]() -> int { HIP_TRY(c, ar.colour(k, c->n_cus, st)); return NERF_OK; });
}

// Zero certification (nerf_render_opts.certify_zero; DESIGN 4.9, protocol: sampling_kernels.hip k_cert_*): a 16-bit pass (f16 or bf16 operands,
// cert_prefilter_f16) over all samples finds (Z) the samples whose density pre-activation is so far below 0 (margin per network,
// c->cert_margin: audited every frame and widened by render_device when the audit's headroom shrinks) that the exact network's density is
// certainly 0 there too, and predicts (C) where each ray's transmittance falls below the reference's 1e-4 cut; the exact kernel evaluates only
// the remaining samples in front of the predicted cut (a device-side list), the exact transmittance confirms the cut (or a second launch
// evaluates the rest).  A certified sample has sigma = 0 => weight 0, a sample behind the cut has weight 0 whatever its density: the frame is
// the plain frame, bit for bit, as long as no certificate is wrong.
// Per network: 16-bit pre-activations of all samples -> plan (list 1, predicted cuts) -> exact kernel on list 1 -> audit -> exact
// transmittance confirms the cuts (list 2 = what is left of the rays it does not) -> exact kernel on list 2.
// a: the plain ray-mode launch of this network in arithmetic dt (eval_net), from which every launch here is derived.
// A batch with per-ray origins (p.origins) hands them to the pre-filter and to the list launches as ray_origins: nothing is expanded into
// points, and the fused pre-filter (NERF_CERTIFY_SEQ_PREFILTER=0), which knows one origin only, gives way to the ray-sequential one.
// far_: only the interval behind a ray's LAST sample depends on it, and no certify kernel's result does: the kernels get
// j.far_cert, the exact per-ray far stays with k_resample and k_composite.
int cert_pass(nerf_ctx *c, const RenderJob &j, const Pass &p, const MlpArgs &a, const DevNet &net, int which, int dt, EvKind kind) {
    const hipStream_t st = j.st;
    const int n_pts = a.n_points, spr = a.samples_per_ray;
    const float *t_in = a.t;
    float *sigma_out = a.sigma_out, *rgb_out = a.rgb_out;
    CertCounters *ctr = c->dev<CertCounters>(BUF_CERT) + (2 * (size_t)p.index + which);
    const unsigned cap = (unsigned)std::min<size_t>(j.cert_cap, (size_t)n_pts);
    // the pre-filter's arithmetic: f16 where the network fits its range (8 x closer to the exact pre-activations: tighter margins, a shorter
    // list), else bf16; a tile of the f16 pass that saw an activation leave the range counts in range_left and render_device goes back to bf16
    const Prefilter &pf = prefilter_of(c->cert_prefilter_f16[which]);
    MlpArgs b = a;
    b.ray_origins = p.origins;
    b.wstream = net.at(pf.stream); b.small_params = net.at(NET_SMALL);
    b.rgb_out = nullptr; b.raw_pre = 1; b.skip_empty = 0; b.skip_counter = nullptr; b.nonfinite = pf.counts_range ? &ctr->range_left : nullptr;
    const EvKind kind_side = which == 0 && !rgb_out ? EV_COARSE_MLP : EV_COLOUR_SIDE;
    int rc = timed(c, st, kind_side, 0, [&]() -> int {
        if (c->cert_seq_prefilter || p.origins) {
            // the pre-filter walks each ray front to back and stops where its own (bf16) transmittance predicts the cut, a little
            // later than k_cert_plan will (depth + 0.5): samples it never reaches stay NaN = "not evaluated" = uncertain
            HIP_TRY(c, hipMemsetAsync(sigma_out, 0xFF, (size_t)n_pts * sizeof(float), st));
            SeqArgs q = seq_args(c, j, p, spr, t_in, sigma_out);
            q.wstream = b.wstream; q.small_params = b.small_params; q.nonfinite = b.nonfinite;
            q.far_ = j.far_cert; q.ray_origins = p.origins;
            q.ray_counter = &ctr->pf_ray_head; q.stats = &ctr->pf_samples;
            q.prefilter = 1; q.prefilter_cut_T = expf(-(c->cert_depth_limit + 0.5f));
            HIP_TRY(c, pf.trunk(q, false, c->n_cus, st));
        } else HIP_TRY(c, pf.fused(b, false, c->n_cus, st));
        CertPlanArgs q{};
        q.pre = sigma_out; q.t = t_in; q.n_rays = p.n_rays; q.spr = spr; q.far_ = j.far_cert;
        q.margin = c->cert_margin[which]; q.depth_limit = c->cert_depth_limit;
        q.audit_mask = c->cert_audit_mask; q.audit_mask_near = c->cert_audit_mask_near;
        q.audit_salt = (unsigned)(j.seed * 0x9E3779B97F4A7C15ull >> 32) + 0x632BE5ABu * p.index + (unsigned)which;
        q.list = c->dev<unsigned int>(BUF_POINT_LIST); q.count = &ctr->list1_len; q.capacity = cap; q.jstar = c->dev<int>(BUF_JSTAR);
        // full evaluations: probable zeros (pre-filter pre-activation below -margin x cert_zero_frac: several times the largest pre-filter error
        // the lego audits see is not needed for a skip -- a positive density among them only keeps its tile's colour heads) and the audited
        // certificates go to the back part of the list, whose all-zero tiles skip the colour head (exact: skip_empty)
        if (rgb_out && c->cert_zero_tiles) { q.count_back = &ctr->list1_back_len; q.zero_threshold = c->cert_margin[which] * c->cert_zero_frac; }
        q.aux = c->dev<unsigned int>(BUF_CERT_AUX); q.aux_count = &ctr->aux_count; q.aux_capacity = (unsigned)j.aux_cap;
        HIP_TRY(c, launch_cert_plan(q, st));
        if (rgb_out) HIP_TRY(c, hipMemsetAsync(rgb_out, 0, (size_t)n_pts * 3 * sizeof(float), st)); // weight 0 either way: 0 * 0
        return NERF_OK;
    });
    if (rc) return rc;
    MlpArgs l = b;
    fill_net(c, net, dt, l); l.raw_pre = 0; l.mode = MLP_MODE_LIST; l.rgb_out = rgb_out; l.n_points = (int)cap;
    l.point_list = c->dev<unsigned int>(BUF_POINT_LIST); l.point_list_count = &ctr->list1_len;
    if (rgb_out && c->cert_zero_tiles) { l.point_list_count_back = &ctr->list1_back_len; l.skip_empty = 1; l.skip_counter = c->dev<unsigned long long>(BUF_SKIP); }
    // points = 0: the list's length is known on the device only (nerf_stats.n_exec_* report it after the frame)
    if (cap > 0 && (rc = timed(c, st, kind, 0, [&]() -> int { HIP_TRY(c, launch_mlp(c, dt, l, rgb_out != nullptr, st)); return NERF_OK; }))) return rc;
    return timed(c, st, kind_side, 0, [&]() -> int {
        HIP_TRY(c, launch_cert_audit(c->dev<unsigned int>(BUF_CERT_AUX), &ctr->aux_count, (unsigned)j.aux_cap, sigma_out, &ctr->audited, c->n_cus, st));
        CertVerifyArgs v{};
        v.t = t_in; v.sigma = sigma_out; v.n_rays = p.n_rays; v.spr = spr; v.far_ = j.far_cert; v.jstar = c->dev<int>(BUF_JSTAR);
        v.list = c->dev<unsigned int>(BUF_POINT_LIST); v.count = &ctr->list2_len; v.capacity = cap; v.fallback_rays = &ctr->fallback_rays;
        HIP_TRY(c, launch_cert_verify(v, st));
        l.point_list_count = &ctr->list2_len; l.point_list_count_back = nullptr;
        if (cap > 0) HIP_TRY(c, launch_mlp(c, dt, l, rgb_out != nullptr, st)); // usually an empty list: the launch returns at once
        return NERF_OK;
    });
}

// steps 2 and 5: network `which` in arithmetic dt over the spr samples per ray at t of the pass's rays; rgb_out == NULL: densities only.
// Four ways: ray-sequential (skip_dead), certified (certify_zero: per-ray origins go along as ray_origins, cert_pass), or plainly -- in ray
// mode from the shared origin (the origin rides in the kernel arguments), or for per-ray origins in points mode behind k_batch_points, which
// expands the samples into points + per-sample directions; points mode forms nothing itself and then runs the same per-column arithmetic:
// the two plain paths carry the same bits.
int eval_net(nerf_ctx *c, const RenderJob &j, const Pass &p, int which, int dt, int spr, const float *t, float *sigma_out, float *rgb_out, EvKind kind) {
    const DevNet &net = c->net[which];
    if (j.seq) return seq_pass(c, j, p, net, dt, spr, t, sigma_out, rgb_out, 3 * (int)p.index + which, kind);
    const hipStream_t st = j.st;
    MlpArgs a{};
    a.ray_dirs = c->dev(BUF_DIRS);
    if (p.origins && !j.certify) a.mode = MLP_MODE_POINTS;
    else { a.mode = MLP_MODE_RAYS; copy3(a.origin, j.origin); }
    fill_net(c, net, dt, a);
    a.n_points = p.n_rays * spr; a.samples_per_ray = spr; a.t = t;
    a.rays_per_row = j.batch ? 0 : p.g.rw; // an image pass is whole rows of the window: the f32 ray-mode launcher may tile its waves over pixel blocks (mlp_layout.h)
    a.sigma_out = sigma_out; a.rgb_out = rgb_out; // the coarse network: sigma only unless its colours are composited (reference discards them, src/lib.rs:404)
    a.skip_empty = j.skip_empty; a.skip_counter = j.skip_empty ? c->dev<unsigned long long>(BUF_SKIP) : nullptr; // only full kernels look at it
    if (which == (c->clock_coarse ? NERF_NET_COARSE : NERF_NET_FINE)) a.clock_out = j.clock_out;
    if (j.certify) return cert_pass(c, j, p, a, net, which, dt, kind);
    bool full = rgb_out != nullptr;
    // the empty-tile vote of a plain render (MlpArgs.empty_vote; exact): every full ray-mode launch of the f32 and split kernels, whatever its
    // mapping.  skip_empty renders keep their own switch with all it means; the 16-bit kernel and points mode keep what they have.
    const bool voted = c->empty_tile_vote && full && a.mode == MLP_MODE_RAYS && !j.skip_empty && dt != NERF_MLP_BF16;
    a.empty_vote = voted ? 1 : 0;
    const bool count_votes = voted && c->debug_empty_tiles && c->buf[BUF_SKIP].p; // NERF_DEBUG_EMPTY_TILES: never on in timed runs
    if (count_votes) {
        a.skip_counter = c->dev<unsigned long long>(BUF_SKIP);
        HIP_TRY(c, hipMemsetAsync(a.skip_counter, 0, sizeof(unsigned long long), st));
    }
    // the coarse cut (MlpArgs.ray_cut; exact): the f32 sampling launch of a plain image render, whose densities go to launch_resample and nowhere
    // else (render_passes) -- not coarse_only, not nf == 0, not a ray batch; skip_dead and certify_zero renders have left above.  The resampler
    // ends the rays at j.far_ (per-ray bounds belong to batches).  nerf_mlp_ray_cut says whether the launch's shape qualifies.
    if (c->coarse_cut && c->buf[BUF_CUT].p && which == NERF_NET_COARSE && !full && dt == NERF_MLP_F32 && a.mode == MLP_MODE_RAYS && !j.batch &&
        !j.coarse_only && j.nf > 0 && sigma_out == c->dev(BUF_SC)) {
        a.cut_counters = c->dev<unsigned int>(BUF_CUT); a.ray_cut_far = j.far_;
        // ... and whether it has the blocks to keep every workgroup busy (nerf_internal.h kCutMinBlocksPerWorkgroup; NERF_COARSE_CUT=2: any number)
        const long long blocks = nerf_mlp_ray_cut(a, full).blocks;
        a.ray_cut = blocks > 0 && (c->coarse_cut >= 2 || blocks >= (long long)nerf_ctx::kCutMinBlocksPerWorkgroup * c->n_cus) ? 1 : 0;
        if (!a.ray_cut) a.cut_counters = nullptr;
    }
    const bool count_cut = a.ray_cut && c->debug_coarse_cut; // NERF_DEBUG_COARSE_CUT: never on in timed runs
    if (count_cut) {
        a.cut_count = 1;
        HIP_TRY(c, hipMemsetAsync(a.cut_counters + 2, 0, sizeof(unsigned long long), st));
    }
    if (p.origins) {
        // only the f32 kernel has a sigma-only points mode: a bf16 sampling pass over expanded points runs the full kernel (the same
        // densities) and leaves its colours in the fine pass's buffer, which that pass overwrites
        if (!full && dt != NERF_MLP_F32) { full = true; a.rgb_out = c->dev(BUF_RGBF); }
        BatchPointsArgs q{};
        q.n_rays = p.n_rays; q.spr = spr; q.origins = p.origins; q.dirs = c->dev(BUF_DIRS); q.t = t;
        q.pts_soa = j.d_pts; q.dirs_aos = j.d_daos;
        a.pts_soa = j.d_pts; a.dirs_aos = j.d_daos;
        int rc;
        if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_batch_points(q, st)); return NERF_OK; }))) return rc;
    }
    // depth ordering (mlp_layout.h DepthOrder): the fine f32 launch of an image pass takes its waves from the pass's depth-sorted pixel blocks;
    // the table is built here, behind the resampler that wrote t, on the render's stream
    if (dt == NERF_MLP_F32 && !p.origins) {
        const nerfmlp::DepthOrder d = nerf_mlp_depth_order(a, full);
        if (d.tiles > 0) {
            int rc;
            if ((rc = c->buf[BUF_ORDER].ensure(c, (size_t)d.points * sizeof(unsigned int)))) return rc;
            DepthOrderArgs q{};
            q.t = t; q.rw = a.rays_per_row; q.spr = spr; q.blocks_x = d.blocks_x; q.blocks = d.blocks; q.table = c->dev<unsigned int>(BUF_ORDER);
            // the fine cut (MlpArgs.fine_cut; exact): this ordered full launch, if it belongs to a plain image render whose sigma and rgb go to
            // launch_composite and nowhere else (render_passes: the fine pass, or the coarse network's of a coarse_only render) -- not a ray batch
            // (per-ray bounds), not a normals render (its stencil pass is a second reader of the pass); skip_dead and certify_zero renders have
            // left above, a skip_empty launch has no table, the stage calls do not come through here.  The compositor ends the rays at j.far_.
            // Only launches with the blocks to keep every workgroup busy (nerf_internal.h kFineCutMinBlocksPerWorkgroup; NERF_FINE_CUT=2: any number).
            if (c->fine_cut && c->buf[BUF_CUT].p && full && a.mode == MLP_MODE_RAYS && !j.batch && !j.normals && rgb_out &&
                (c->fine_cut >= 2 || (long long)d.blocks >= (long long)nerf_ctx::kFineCutMinBlocksPerWorkgroup * c->n_cus) &&
                (which == NERF_NET_FINE ? sigma_out == c->dev(BUF_SF) && rgb_out == c->dev(BUF_RGBF)
                                        : j.coarse_only && sigma_out == c->dev(BUF_SC) && rgb_out == c->dev(BUF_RGBC))) {
                if ((rc = c->buf[BUF_ORDER_FLAGS].ensure(c, (size_t)d.blocks * sizeof(unsigned int)))) return rc;
                q.flags = c->dev<unsigned int>(BUF_ORDER_FLAGS);
                a.fine_cut = 1; a.order_flags = q.flags; a.cut_counters = c->dev<unsigned int>(BUF_CUT); a.ray_cut_far = j.far_;
                if (c->debug_fine_cut) { // NERF_DEBUG_FINE_CUT: never on in timed runs
                    a.cut_count = 1;
                    HIP_TRY(c, hipMemsetAsync(a.cut_counters + 2, 0, sizeof(unsigned long long), st));
                }
            }
            if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_depth_order(q, st)); return NERF_OK; }))) return rc;
            a.order_table = c->dev<unsigned int>(BUF_ORDER);
        }
    }
    const int rc = timed(c, st, kind, (uint64_t)a.n_points, [&]() -> int { HIP_TRY(c, launch_mlp(c, dt, a, full, st)); return NERF_OK; });
    if (!rc && count_cut) { // the read synchronises, as nerf_zskip_print does
        unsigned long long skipped = 0;
        HIP_TRY(c, hipMemcpyAsync(&skipped, a.cut_counters + 2, sizeof skipped, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        fprintf(stderr, "nerf coarse cut: nerf_mlp_kernel<sigma,rays> tiles_skipped=%llu tiles=%d blocks=%d\n", skipped,
                (a.n_points + nerfmlp::kPointsPerBlock - 1) / nerfmlp::kPointsPerBlock, nerf_mlp_ray_cut(a, full).blocks);
    }
    if (!rc && a.fine_cut && a.cut_count) {
        unsigned long long skipped = 0;
        HIP_TRY(c, hipMemcpyAsync(&skipped, a.cut_counters + 2, sizeof skipped, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        fprintf(stderr, "nerf fine cut: nerf_mlp_kernel<full,rays> tiles_skipped=%llu tiles=%d blocks=%d\n", skipped,
                (a.n_points + nerfmlp::kPointsPerBlock - 1) / nerfmlp::kPointsPerBlock, nerf_mlp_fine_cut(a, full).blocks);
    }
    if (rc || !count_votes) return rc;
    unsigned long long tiles = 0; // the read synchronises, as nerf_zskip_print does
    HIP_TRY(c, hipMemcpyAsync(&tiles, a.skip_counter, sizeof tiles, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    static const char *const kernels[4] = {"nerf_mlp_kernel<full,rays>", "", "nerf_mlp_kernel_bf16x3<full,rays>", "nerf_mlp_kernel_f16x2<full,rays>"}; // by NERF_MLP_*
    fprintf(stderr, "nerf empty tiles: %s tiles_skipped=%llu tiles=%d\n", kernels[dt], tiles, (a.n_points + nerfmlp::kPointsPerBlock - 1) / nerfmlp::kPointsPerBlock);
    return NERF_OK;
}

// hybrid_sampling, after the first resample ra: the coarse densities came from the split arithmetic.  Redo, in exact f32, the rays with a
// draw in a light CDF bin (their sample positions are the ill-conditioned ones) and resample just those: same positions as the f32 path.
// hctr: the pass's third SeqCounters; its live_count is the number of flagged rays
int hybrid_redo(nerf_ctx *c, const RenderJob &j, const Pass &p, const ResampleArgs &ra, SeqCounters *hctr) {
    const hipStream_t st = j.st;
    const DevNet &NC = c->net[NERF_NET_COARSE];
    SeqArgs q = seq_args(c, j, p, j.nc, c->dev(BUF_TC), c->dev(BUF_SC));
    fill_net(c, NC, NERF_MLP_F32, q);
    q.ray_counter = &hctr->ray_head; q.stats = &hctr->evaluated;
    q.live_count = nullptr; // hctr->live_count is the LENGTH of the ray list below: this launch never exports (no colour head)
    q.ray_list = c->dev<unsigned int>(BUF_FLAG_LIST); q.ray_list_count = &hctr->live_count; q.zero_fill_after_cut = 1;
    int rc;
    if ((rc = timed(c, st, EV_COARSE_MLP, 0, [&]() -> int { HIP_TRY(c, arith_of(NERF_MLP_F32).trunk(q, false, c->n_cus, st)); return NERF_OK; }))) return rc;
    ResampleArgs rb = ra;
    rb.flag_tau = 0.0f; rb.flag_count = nullptr; rb.flag_list = nullptr;
    rb.ray_list = c->dev<unsigned int>(BUF_FLAG_LIST); rb.ray_list_count = &hctr->live_count;
    return timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_resample(rb, st)); return NERF_OK; });
}

// The normals of the pass (j.normals != NULL), from the weights the compositing launch left in nw.w (t: the composited samples' positions):
//     count + scan + list (3 launches) -> [8 bytes to the host] -> stencil -> sigma-only MLP over 6 L points -> reduce
// The live total L of a pass goes back to the host -- ONE SMALL COPY AND ONE STREAM SYNCHRONISATION PER PASS, as mesh_extract reads
// its counts: it sizes the stencil workspace (16 B per point, grown on demand) and the launches that follow; a pass with L = 0 launches
// nothing further and writes zero normals.  The network differentiated is the one composited, always in f32.
int normals_pass(nerf_ctx *c, const RenderJob &j, const Pass &p, const DevNet &net, const float *t) {
    if (!j.normals) return NERF_OK;
    const hipStream_t st = j.st;
    const NormalWorkspace &nw = j.nw;
    const int n_rays = p.n_rays, n_comp = j.n_comp;
    int rc;
    NormalListArgs la{nw.w, n_rays, n_comp, nw.count, nw.base, nw.bsum, nw.totals, nw.list};
    if ((rc = timed(c, st, EV_NORMAL_SMALL, 0, [&]() -> int { HIP_TRY(c, launch_normal_list(la, st)); return NERF_OK; }))) return rc;
    uint32_t totals[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(totals, nw.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const size_t L = totals[0];
    c->normal_live += L; c->normal_samples += (uint64_t)n_rays * (uint64_t)n_comp;
    float *out = j.normals + 3 * p.r0;
    if (L == 0) { HIP_TRY(c, hipMemsetAsync(out, 0, (size_t)n_rays * 3 * sizeof(float), st)); return NERF_OK; }
    if (L > (size_t)n_rays * (size_t)n_comp) return fail(c, NERF_ERR_HIP, "normals: the live count exceeds the pass's samples");
    if ((rc = c->buf[BUF_STENCIL].ensure(c, 6 * L * 4 * sizeof(float)))) return rc;
    float *d_spts = c->dev(BUF_STENCIL), *d_ssig = d_spts + 18 * L;
    NormalStencilArgs sa{};
    sa.n_live = (uint32_t)L; sa.h = j.h; sa.list = nw.list; sa.spr = n_comp; sa.origins = p.origins; sa.dirs = c->dev(BUF_DIRS); sa.t = t; sa.pts = d_spts;
    if (!p.origins) copy3(sa.origin, j.origin);
    if ((rc = timed(c, st, EV_NORMAL_SMALL, 0, [&]() -> int { HIP_TRY(c, launch_normal_stencil(sa, st)); return NERF_OK; }))) return rc;
    if ((rc = timed(c, st, EV_NORMAL_SIGMA, (uint64_t)(6 * L), [&]() -> int { HIP_TRY(c, launch_sigma_points(c, net, d_spts, 6 * L, d_ssig, st)); return NERF_OK; }))) return rc;
    NormalReduceArgs ra{n_rays, (uint32_t)L, nw.count, nw.base, nw.list, nw.w, d_spts, d_ssig, out};
    return timed(c, st, EV_NORMAL_SMALL, 0, [&]() -> int { HIP_TRY(c, launch_normal_reduce(ra, st)); return NERF_OK; });
}

// The quantile depths of the pass (j.n_q > 0) from the weights the compositing launch left in j.w_surface (t: the composited samples'
// positions), and for a points render the compaction of the pass's kept rays behind those of the passes before it: the running offset is
// a word on the device, nothing comes back to the host.  Runs behind normals_pass, whose normals the point records carry.
int surface_pass(nerf_ctx *c, const RenderJob &j, const Pass &p, const float *t) {
    if (!j.n_q) return NERF_OK;
    const hipStream_t st = j.st;
    RayQuantileArgs qa{};
    qa.n_rays = p.n_rays; qa.n = j.n_comp; qa.w = j.w_surface; qa.t = t; qa.n_q = j.n_q;
    for (int k = 0; k < j.n_q; ++k) qa.q[k] = j.quant[k];
    qa.out = j.depth_q + p.r0; qa.plane_stride = j.depth_q_stride;
    int rc;
    if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_ray_quantiles(qa, st)); return NERF_OK; }))) return rc;
    if (!j.points) return NERF_OK;
    PointGatherArgs g = j.pg;
    g.n_rays = p.n_rays; g.first_ray = (uint32_t)p.r0;
    g.origins = p.origins; copy3(g.origin, j.origin);
    g.dirs = c->dev(BUF_DIRS); g.depth_q = j.depth_q + p.r0; g.rgb = j.out + 3 * p.r0; g.opacity = j.opacity + p.r0;
    g.normals = j.normals ? j.normals + 3 * p.r0 : nullptr;
    return timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_point_gather(g, st)); return NERF_OK; });
}

// The loop over passes: everything a render launches between its driver's allocations and its counters' read-back.
int render_passes(nerf_ctx *c, const RenderJob &j, uint32_t *n_passes) {
    const hipStream_t st = j.st;
    int rc;
    if ((j.skip_empty || j.certify) && c->buf[BUF_SKIP].p) HIP_TRY(c, hipMemsetAsync(c->buf[BUF_SKIP].p, 0, sizeof(unsigned long long), st));
    if (watches_range(c, j)) HIP_TRY(c, hipMemsetAsync(c->buf[BUF_NONFINITE].p, 0, sizeof(unsigned int), st));
    const DevNet &NC = c->net[NERF_NET_COARSE], &NF = c->net[NERF_NET_FINE];
    uint32_t passes = 0;
    for (size_t r0 = 0; r0 < j.n_rays; r0 += j.pass_rays, ++passes) {
        Pass p{};
        p.index = passes; p.r0 = r0; p.n_rays = (int)std::min(j.pass_rays, j.n_rays - r0);
        if ((rc = prepare_rays(c, j, p))) return rc;
        if ((rc = eval_net(c, j, p, NERF_NET_COARSE, j.dtype_coarse, j.nc, c->dev(BUF_TC), c->dev(BUF_SC), j.coarse_only ? c->dev(BUF_RGBC) : nullptr,
                           j.coarse_only ? j.kind_colour : EV_COARSE_MLP))) return rc;
        CompositeArgs ca{};
        ca.n_rays = p.n_rays; ca.far_ = j.far_; ca.far_per_ray = j.d_far; ca.out = j.out + 3 * r0;
        ca.depth = j.depth ? j.depth + r0 : nullptr; ca.opacity = j.opacity ? j.opacity + r0 : nullptr;
        if (j.background) { ca.use_bg = 1; copy3(ca.bg, j.background); }
        if (j.normals) ca.w_out = j.nw.w;
        else if (j.n_q) ca.w_out = j.w_surface;
        if (j.coarse_only) {
            ca.n = j.nc; ca.t = c->dev(BUF_TC); ca.sigma = c->dev(BUF_SC); ca.rgb = c->dev(BUF_RGBC);
            if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_composite(ca, st)); return NERF_OK; }))) return rc;
            if ((rc = normals_pass(c, j, p, NC, c->dev(BUF_TC)))) return rc;
            if ((rc = surface_pass(c, j, p, c->dev(BUF_TC)))) return rc;
            continue;
        }
        const float *t_fine = c->dev(BUF_TC);
        if (j.nf > 0) {
            ResampleArgs ra{};
            ra.g = p.g; ra.n_rays = p.n_rays; ra.nc = j.nc; ra.nf = j.nf; ra.far_ = j.far_; ra.far_per_ray = j.d_far;
            ra.seed_lo = (uint32_t)j.seed; ra.seed_hi = (uint32_t)(j.seed >> 32);
            ra.t_coarse = c->dev(BUF_TC); ra.sigma_coarse = c->dev(BUF_SC); ra.t_fine = c->dev(BUF_TF);
            ra.pixel_index = p.rng;
            SeqCounters *hctr = j.seq ? c->dev<SeqCounters>(BUF_SEQ) + (3 * (size_t)passes + 2) : nullptr;
            if (j.hybrid) { ra.flag_tau = c->hybrid_tau; ra.flag_count = &hctr->live_count; ra.flag_list = c->dev<unsigned int>(BUF_FLAG_LIST); }
            if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_resample(ra, st)); return NERF_OK; }))) return rc;
            if (j.hybrid && (rc = hybrid_redo(c, j, p, ra, hctr))) return rc;
            t_fine = c->dev(BUF_TF);
        }
        if (j.clock_out) c->clock_valid = true;
        if ((rc = eval_net(c, j, p, NERF_NET_FINE, j.dtype, j.M, t_fine, c->dev(BUF_SF), c->dev(BUF_RGBF), j.kind_colour))) return rc;
        ca.n = j.M; ca.t = t_fine; ca.sigma = c->dev(BUF_SF); ca.rgb = c->dev(BUF_RGBF);
        if ((rc = timed(c, st, EV_OTHER, 0, [&]() -> int { HIP_TRY(c, launch_composite(ca, st)); return NERF_OK; }))) return rc;
        if ((rc = normals_pass(c, j, p, NF, t_fine))) return rc;
        if ((rc = surface_pass(c, j, p, t_fine))) return rc;
    }
    *n_passes = passes;
    return NERF_OK;
}

// What the audit of a certify_zero frame found (per network: 0 coarse, 1 fine), read from the device after the frame.
struct CertOutcome {
    uint64_t audited[2] = {0, 0}, violations[2] = {0, 0};
    float headroom[2] = {INFINITY, INFINITY}; // min over the audited certificates of -(exact pre-activation)
    float max_err[2] = {0.0f, 0.0f};          // max over them of |bf16 - exact pre-activation|
    uint64_t listed[2] = {0, 0};      // samples the exact kernel evaluated (both launches, audited certificates included)
    uint64_t fallback_rays = 0;       // rays whose predicted cut the exact transmittance did not confirm
    uint64_t range_left[2] = {0, 0};  // f16 pre-filter: wave tiles in which an activation left the f16 range (the frame's certificates are void)
    uint64_t list_need = 0;           // largest list any pass wanted ...
    uint64_t list_capacity = 0;       // ... and what it had
    uint64_t pass_samples = 0;        // samples of the largest network pass (the list's worst case)
    bool used[2] = {false, false};
};

// the audit's outcome decides whether this frame stands (render_device): certify_zero renders synchronise the stream
int read_cert_outcome(nerf_ctx *c, const RenderJob &j, uint32_t passes, CertOutcome *cert) {
    HIP_TRY(c, hipStreamSynchronize(j.st));
    std::vector<CertCounters> h((size_t)passes * 2);
    HIP_TRY(c, hipMemcpy(h.data(), c->dev(BUF_CERT), h.size() * sizeof(CertCounters), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < passes * 2; ++k) {
        const CertCounters &q = h[k];
        const int w = (int)(k & 1);
        if (w == 1 && j.coarse_only) continue;
        cert->used[w] = true;
        const uint64_t list1 = (uint64_t)q.list1_len + q.list1_back_len;
        cert->listed[w] += std::min<uint64_t>(list1, cert->list_capacity) + std::min<uint64_t>(q.list2_len, cert->list_capacity);
        cert->list_need = std::max<uint64_t>(cert->list_need, std::max<uint64_t>(list1, q.list2_len));
        cert->audited[w] += q.audited; cert->violations[w] += q.violations;
        if (q.audited) {
            const unsigned bits = 0x7f800000u - q.headroom_code;
            float hr, er;
            memcpy(&hr, &bits, sizeof hr); memcpy(&er, &q.max_err_bits, sizeof er);
            cert->headroom[w] = std::min(cert->headroom[w], hr); cert->max_err[w] = std::max(cert->max_err[w], er);
        }
        cert->fallback_rays += q.fallback_rays;
        cert->range_left[w] += q.range_left;
    }
    return NERF_OK;
}

// The stats of a finished render (stats != NULL: synchronises the stream): the part every render has, then what the job's modes counted.
int finish_stats(nerf_ctx *c, const RenderJob &j, uint32_t passes, nerf_stats *stats, const CertOutcome *cert) {
    if (!stats) return NERF_OK;
    HIP_TRY(c, hipStreamSynchronize(j.st));
    memset(stats, 0, sizeof *stats);
    stats->n_rays = j.n_rays;
    stats->n_passes = passes;
    stats->n_coarse_points = stats->n_rays * (uint64_t)j.nc;                       // nominal: every sample of every ray
    stats->n_fine_points = j.coarse_only ? 0 : stats->n_rays * (uint64_t)j.M;
    double ms_normal_sigma = 0.0, ms_normal_small = 0.0;
    for (const auto &p : c->last_render) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, p.a, p.b));
        if (p.kind == EV_COARSE_MLP) { stats->ms_coarse_mlp += ms; stats->n_mlp_launches++; }
        else if (p.kind == EV_IMAGE_COLOUR || p.kind == EV_COLOUR_SIDE || p.kind == EV_BATCH_COLOUR) { // the colour-producing launch and its side launches
            stats->n_mlp_launches++;
            if (j.coarse_only) stats->ms_coarse_mlp += ms; else stats->ms_fine_mlp += ms;
        } else stats->ms_other += ms; // EV_NORMAL_* too: a normals render's own launches are neither network pass of the colour
        if (p.kind == EV_NORMAL_SIGMA) ms_normal_sigma += ms; else if (p.kind == EV_NORMAL_SMALL) ms_normal_small += ms;
    }
    if (!c->last_render.empty()) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->last_render.front().a, c->last_render.back().b));
        stats->ms_total = ms;
    }
    if (j.normals && c->debug_normals)
        fprintf(stderr, "nerf normals: %llu live of %llu composited samples, sigma launches %.3f ms over %llu points, other normal kernels %.3f ms\n",
                (unsigned long long)c->normal_live, (unsigned long long)c->normal_samples, ms_normal_sigma, (unsigned long long)(6 * c->normal_live),
                ms_normal_small);
    if (watches_range(c, j)) {
        unsigned int bad = 0;
        HIP_TRY(c, hipMemcpy(&bad, c->buf[BUF_NONFINITE].p, sizeof bad, hipMemcpyDeviceToHost));
        stats->n_nonfinite_points = bad;
    }
    if ((j.skip_empty || j.certify) && c->buf[BUF_SKIP].p) { // certify_zero: all-zero tiles of the list's back part (probable zeros, audited certificates)
        unsigned long long tiles = 0;
        HIP_TRY(c, hipMemcpy(&tiles, c->buf[BUF_SKIP].p, sizeof tiles, hipMemcpyDeviceToHost));
        stats->n_colour_skipped_points = (uint64_t)tiles * nerfmlp::kPointsPerBlock;
    }
    // evaluations actually executed
    const uint64_t n_colour = j.coarse_only ? stats->n_coarse_points : stats->n_fine_points;
    stats->n_exec_coarse_trunk = stats->n_coarse_points;
    stats->n_exec_fine_trunk = stats->n_fine_points;
    stats->n_exec_colour = n_colour - stats->n_colour_skipped_points;
    if (j.certify && cert) { // samples the exact kernel evaluated = the lengths of the lists (audited certificates included)
        const uint64_t listed = j.coarse_only ? cert->listed[0] : cert->listed[1];
        stats->n_exec_coarse_trunk = cert->listed[0];
        stats->n_exec_fine_trunk = j.coarse_only ? 0 : cert->listed[1];
        stats->n_exec_colour = listed - std::min<uint64_t>(stats->n_colour_skipped_points, listed);
        stats->n_certify_audited = cert->audited[0] + cert->audited[1];
        stats->n_certify_violations = cert->violations[0] + cert->violations[1];
        stats->n_certify_fallback_rays = (uint32_t)std::min<uint64_t>(cert->fallback_rays, 0xffffffffu);
        for (int w = 0; w < 2; ++w) { stats->certify_margin[w] = c->cert_margin[w]; stats->certify_headroom[w] = cert->headroom[w]; stats->certify_max_error[w] = cert->max_err[w]; }
    }
    if (j.seq) {
        std::vector<SeqCounters> h((size_t)passes * 3);
        HIP_TRY(c, hipMemcpy(h.data(), c->dev(BUF_SEQ), h.size() * sizeof(SeqCounters), hipMemcpyDeviceToHost));
        uint64_t evaluated[3] = {0, 0, 0}, live = 0; // samples the trunk launches evaluated (a ray's last chunk may be partial)
        for (uint32_t k = 0; k < passes * 3; ++k) {
            evaluated[k % 3] += h[k].evaluated;
            if (k % 3 == 2) stats->n_hybrid_rays += h[k].live_count; // flagged rays redone in f32
            else live += h[k].live_count;
        }
        stats->n_exec_coarse_trunk = evaluated[0] + evaluated[2];
        stats->n_exec_fine_trunk = j.coarse_only ? 0 : evaluated[1];
        stats->n_exec_colour = live;
        stats->n_colour_skipped_points = n_colour - live;
    }
    if (stats->n_nonfinite_points) { // the result is WRONG there (f16 overflow yields finite garbage, not NaN): never return it as a success
        char msg[320];
        snprintf(msg, sizeof msg, "%llu evaluations: an operand left the range of the split arithmetic (NERF_MLP_F16X2: |activation| <= 65504) or a "
                 "density was not finite; the %s is not usable -- use NERF_MLP_BF16X3 or NERF_MLP_F32", (unsigned long long)stats->n_nonfinite_points, j.what);
        return fail(c, NERF_ERR_STATE, msg);
    }
    return NERF_OK;
}

// ---- image renders --------------------------------------------------------------------------------------------------------------------
// the mode switches of an image render and the combinations the kernels exist for
int check_image_modes(nerf_ctx *c, const nerf_render_opts *o) {
    const int dtype = o->mlp_dtype;
    if (o->skip_empty != 0 && o->skip_empty != 1) return fail(c, NERF_ERR_INVALID, "skip_empty must be 0 or 1");
    if (o->skip_dead != 0 && o->skip_dead != 1) return fail(c, NERF_ERR_INVALID, "skip_dead must be 0 or 1");
    const bool seq = o->skip_dead != 0;
    if (o->hybrid_sampling != 0 && o->hybrid_sampling != 1) return fail(c, NERF_ERR_INVALID, "hybrid_sampling must be 0 or 1");
    if (o->certify_zero != 0 && o->certify_zero != 1) return fail(c, NERF_ERR_INVALID, "certify_zero must be 0 or 1");
    if (o->certify_zero && (dtype == NERF_MLP_BF16 || seq || o->skip_empty))
        return fail(c, NERF_ERR_INVALID, "certify_zero needs mlp_dtype F32, BF16X3 or F16X2 and neither skip_empty nor skip_dead");
    if (o->hybrid_sampling && !(seq && !o->coarse_only && dtype != NERF_MLP_BF16)) // bf16 is its own arithmetic: there are no f32 sample positions to protect
        return fail(c, NERF_ERR_INVALID, "hybrid_sampling needs skip_dead = 1, mlp_dtype F32, BF16X3 or F16X2, and a hierarchical render");
    return NERF_OK;
}

// The pixels a render covers: the crop window, or one band of its rows (multi-GPU): contiguous bands are just a shorter window; striped
// bands keep the window and map band-local rows to window rows in the ray generator (sampling_kernels.hip ray_row)
struct Window { int s, x0, y0, cw, ch, stripe; };
int image_window(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, Window *w) {
    w->s = o->ssaa > 1 ? o->ssaa : 1;
    w->x0 = 0; w->y0 = 0; w->cw = cam->nx; w->ch = cam->ny; w->stripe = 0;
    if (o->crop_w > 0 || o->crop_h > 0) { w->x0 = o->crop_x0; w->y0 = o->crop_y0; w->cw = o->crop_w; w->ch = o->crop_h; }
    if (w->cw <= 0 || w->ch <= 0 || w->x0 < 0 || w->y0 < 0 || w->x0 + w->cw > cam->nx || w->y0 + w->ch > cam->ny)
        return fail(c, NERF_ERR_INVALID, "crop window outside the frame");
    if (o->band_count > 1) {
        if (o->band_index < 0 || o->band_index >= o->band_count || o->band_stripe_rows < 0) return fail(c, NERF_ERR_INVALID, "band_index / band_count / band_stripe_rows out of range");
        const int rows = band_rows(w->ch, o->band_index, o->band_count, o->band_stripe_rows);
        if (rows <= 0) return fail(c, NERF_ERR_INVALID, "this band has no rows (more bands than rows)");
        if (o->band_stripe_rows == 0) w->y0 += band_first_row(w->ch, o->band_index, o->band_count);
        else w->stripe = o->band_stripe_rows;
        w->ch = rows;
    } else if (o->band_count < 0) return fail(c, NERF_ERR_INVALID, "band_count must be >= 0");
    return NERF_OK;
}

// skip_dead in a split arithmetic or in bf16 (two launches): the compacted trunk outputs are sized for the worst case (every sample
// of a pass live; 1 KiB each as f32 tiles, 512 B as packed bf16).  The f32 kernel compacts in LDS and runs its colour passes in the
// same launch: no buffer, no extra passes.
bool exports_h8(const RenderJob &j) { return j.seq && arith_of(j.dtype).h8_sample_bytes > 0; }

// the rays per pass that buffer's budget allows (called with the export mutex held)
int export_budget(nerf_ctx *c, const RenderJob &j, int RW, size_t *pass_cap) {
    const size_t h8_sample_bytes = arith_of(j.dtype).h8_sample_bytes;
    size_t budget = c->max_export_bytes, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) // never more than half of what the device can still give (plus what we already hold)
        budget = std::min(budget, (free_b + c->buf[BUF_H8].bytes) / 2);
    const size_t row_bytes = (size_t)RW * j.M * h8_sample_bytes;
    if (row_bytes > budget) {
        char msg[256];
        snprintf(msg, sizeof msg, "skip_dead in this arithmetic exports %zu B per sample: one ray row of this render (%d rays x %d samples) needs "
                 "%zu MiB, the budget is %zu MiB (NERF_MAX_EXPORT_BYTES, free device memory / 2); render a narrower crop or use NERF_MLP_F32",
                 h8_sample_bytes, RW, j.M, row_bytes >> 20, budget >> 20);
        return fail(c, NERF_ERR_INVALID, msg);
    }
    *pass_cap = std::min<size_t>(*pass_cap, budget / ((size_t)j.M * h8_sample_bytes));
    return NERF_OK;
}

// skip_dead: the counters, one SeqCounters per MLP launch, cleared; the export buffer (which releases h8_lock); the hybrid redo's ray list
int reserve_seq(nerf_ctx *c, const RenderJob &j, size_t n_passes, std::unique_lock<std::mutex> &h8_lock) {
    int rc;
    const size_t slots = n_passes * 3; // per pass: coarse, fine, hybrid f32 redo of the coarse pass
    if ((rc = c->buf[BUF_SEQ].ensure(c, slots * sizeof(SeqCounters)))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->dev(BUF_SEQ), 0, slots * sizeof(SeqCounters), j.st));
    const size_t pass_samples = j.pass_rays * (size_t)j.M;
    if (exports_h8(j)) {
        const size_t need = arith_of(j.dtype).h8_bytes(pass_samples);
        DevBuf &h8 = c->buf[BUF_H8];
        if (need < h8.bytes / 4 && (rc = h8.release(c))) return rc; // a much smaller render: give the big buffer back
        if ((rc = h8.ensure(c, need))) return rc;
        if ((rc = c->buf[BUF_SLOT_POINT].ensure(c, (pass_samples + 256) * sizeof(unsigned int)))) return rc;
        h8_lock.unlock();
    }
    if (j.hybrid && (rc = c->buf[BUF_FLAG_LIST].ensure(c, j.pass_rays * sizeof(unsigned int)))) return rc;
    return NERF_OK;
}

// certify_zero: the sample list, the predicted cuts, the audit records and the counters (cleared); sets j.cert_cap and j.aux_cap
int reserve_certify(nerf_ctx *c, RenderJob &j, size_t n_pass, CertOutcome *cert) {
    int rc;
    if (cert_plan_lds_bytes(j.M, nullptr) > 159 * 1024) return fail(c, NERF_ERR_INVALID, "certify_zero: too many samples per ray");
    const size_t pass_samples = j.pass_rays * (size_t)j.M;
    // the list is sized from what earlier frames needed (c->cert_list_frac of the samples, +25 %): if a pass wants more, the entries
    // beyond the capacity are counted, not stored, and render_device renders the frame again with a list that fits
    // (up to 64 MiB the list simply holds every sample: small renders -- a central crop lists 70 % of its samples -- never take that path)
    j.cert_cap = pass_samples <= ((size_t)16 << 20) ? pass_samples : std::min<size_t>(pass_samples, (size_t)((double)pass_samples * c->cert_list_frac) + 4096);
    if ((rc = c->buf[BUF_POINT_LIST].ensure(c, j.cert_cap * sizeof(unsigned int)))) return rc;
    j.cert_cap = std::min<size_t>(pass_samples, c->buf[BUF_POINT_LIST].bytes / sizeof(unsigned int)); // an earlier, larger allocation is kept
    if ((rc = c->buf[BUF_JSTAR].ensure(c, j.pass_rays * sizeof(int)))) return rc;
    j.aux_cap = 2 * (pass_samples / ((size_t)std::min(c->cert_audit_mask, c->cert_audit_mask_near) + 1)) + 4096; // more than the audit can select: a certificate that does not fit is not audited
    if ((rc = c->buf[BUF_CERT_AUX].ensure(c, j.aux_cap * 2 * sizeof(unsigned int)))) return rc;
    if ((rc = c->buf[BUF_CERT].ensure(c, 2 * n_pass * sizeof(CertCounters)))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->dev(BUF_CERT), 0, 2 * n_pass * sizeof(CertCounters), j.st));
    if (cert) { cert->list_capacity = j.cert_cap; cert->pass_samples = pass_samples; }
    return NERF_OK;
}

// One attempt at an image (render_device decides whether a certify_zero frame stands).  Passes are whole ray rows of the window.
int render_once(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, float *d_out, float *d_depth, float *d_opacity, hipStream_t st,
                nerf_stats *stats, CertOutcome *cert, const float *background) {
    int rc;
    if ((rc = check_camera(c, cam))) return rc;
    if (!o) return fail(c, NERF_ERR_INVALID, "opts is NULL");
    if (!d_out) return fail(c, NERF_ERR_INVALID, "output pointer is NULL");
    if ((rc = check_sample_plan(c, o, PLAN_COUNTS))) return rc;
    if ((rc = check_image_modes(c, o))) return rc;
    if ((rc = check_sample_plan(c, o, PLAN_NETWORKS))) return rc;
    Window w;
    if ((rc = image_window(c, cam, o, &w))) return rc;
    if ((rc = check_sample_plan(c, o, PLAN_LIMITS))) return rc;
    RenderJob j{};
    plan_job(c, o, j);
    j.near_ = cam->near_; j.far_ = cam->far_; j.far_cert = j.far_; j.background = background;
    j.kind_colour = EV_IMAGE_COLOUR; j.what = "frame"; j.st = st;
    j.skip_empty = o->skip_empty; j.seq = o->skip_dead != 0; j.certify = o->certify_zero != 0;
    j.hybrid = o->hybrid_sampling != 0 && j.nf > 0; // without resampling there is nothing to protect
    j.clock_out = c->dev<unsigned long long>(BUF_CLOCK); // NULL unless NERF_DEBUG_CLOCK=1
    copy3(j.origin, cam->pos);
    const int s = w.s, RW = w.cw * s, RH = w.ch * s, RX0 = w.x0 * s, RY0 = w.y0 * s;
    size_t pass_cap = pass_capacity(c, j.M);
    // Budget and allocation of the export buffer are ONE critical section per process: contexts that share a device (nerf_render_image_multi's
    // worker threads) would otherwise each claim half of the same free memory and fail in hipMalloc.  A context keeps its buffer while
    // later renders fit; a render that needs less than a quarter of it gives it back (shrinks).
    static std::mutex h8_mu;
    std::unique_lock<std::mutex> h8_lock(h8_mu, std::defer_lock);
    if (exports_h8(j)) {
        h8_lock.lock();
        if ((rc = export_budget(c, j, RW, &pass_cap))) return rc;
    }
    if ((size_t)RW > pass_cap && (size_t)RW * j.M > (size_t)0x3fffffff) return fail(c, NERF_ERR_INVALID, "ray row too wide for one pass");
    const size_t rows_per_pass = std::max<size_t>(1, std::min<size_t>(RH, pass_cap / (size_t)RW));
    j.n_rays = (size_t)RW * RH; j.pass_rays = rows_per_pass * RW;
    if ((rc = ensure_workspace(c, j.pass_rays, j.nc, j.M, j.coarse_only))) return rc;
    j.out = d_out; j.depth = d_depth; j.opacity = d_opacity;
    if (s > 1) {
        if ((rc = c->buf[BUF_RAYFB].ensure(c, (size_t)RW * RH * 3 * sizeof(float)))) return rc;
        j.out = c->dev(BUF_RAYFB);
        if (d_depth || d_opacity) { // ray-level maps, one plane each, box-filtered like the colour below
            if ((rc = c->buf[BUF_RAYAUX].ensure(c, (size_t)RW * RH * 2 * sizeof(float)))) return rc;
            j.depth = d_depth ? c->dev(BUF_RAYAUX) : nullptr;
            j.opacity = d_opacity ? c->dev(BUF_RAYAUX) + (size_t)RW * RH : nullptr;
        }
    }
    const size_t n_passes_total = ((size_t)RH + rows_per_pass - 1) / rows_per_pass;
    if (j.seq && (rc = reserve_seq(c, j, n_passes_total, h8_lock))) return rc;
    if (j.certify && (rc = reserve_certify(c, j, n_passes_total, cert))) return rc;
    recycle_render(c);
    recycle_dominant(c, 4096); // bound the backlog if the caller never queries
    j.g = make_raygen(*cam, s);
    j.g.rx0 = RX0; j.g.rw = RW; j.g.ry0 = w.stripe > 0 ? 0 : RY0;
    if (w.stripe > 0) { j.g.stripe = w.stripe * s; j.g.stripe_n = o->band_count; j.g.stripe_i = o->band_index; j.g.stripe_y0 = RY0; }
    uint32_t passes = 0;
    if ((rc = render_passes(c, j, &passes))) return rc;
    if (s > 1 && (rc = timed(c, st, EV_OTHER, 0, [&]() -> int {
            HIP_TRY(c, launch_box_downsample(c->dev(BUF_RAYFB), d_out, w.cw, w.ch, s, 3, st));
            if (d_depth) HIP_TRY(c, launch_box_downsample(j.depth, d_depth, w.cw, w.ch, s, 1, st));
            if (d_opacity) HIP_TRY(c, launch_box_downsample(j.opacity, d_opacity, w.cw, w.ch, s, 1, st));
            return NERF_OK;
        }))) return rc;
    // the dominant-kernel events also feed nerf_kernel_time_query: from here on c->dominant owns them (a render that returned early above
    // never gets here, and the next recycle_render returns its pairs to the pool with the others)
    for (auto &p : c->last_render)
        if (p.kind == EV_IMAGE_COLOUR) { p.dominant = true; c->dominant.push_back(p); }
    if (cert && (rc = read_cert_outcome(c, j, passes, cert))) return rc;
    return finish_stats(c, j, passes, stats, cert);
}

// ---- ray batches (nerf_render_rays) -------------------------------------------------------------------------------------
// What the header's contract needs beside render_once: the rays are the caller's, so there is no camera, no window and none of the modes
// tied to either; a pass is at most max_rays_per_pass rays (rays * samples <= 0x3fffffff, as above).
// q: a device request, already checked (check_request), with h_origin set when n_origins == 1; asynchronous on q.st unless q.stats or
// q.want_normals (normals: n_rays x 3; the compositing launch then also hands out its weights, and normals_pass follows it in every pass).
// cert != NULL: one attempt at a certified batch (run_rays' retry loop decides whether it stands) -- zero certification inside every pass,
// per-ray origins as ray_origins of the certified kernels (no expansion, no 24-byte-per-sample workspace); synchronises q.st, because the
// audit is read on the host.
int render_rays_device(nerf_ctx *c, const RayRequest &q, CertOutcome *cert) {
    int rc;
    if ((rc = check_sample_plan(c, q.opts, PLAN_NETWORKS))) return rc;
    RenderJob j{};
    plan_job(c, q.opts, j);
    j.near_ = q.near_; j.far_ = q.far_; j.background = q.background;
    j.out = q.rgb; j.depth = q.depth; j.opacity = q.opacity;
    // events: all owned by last_render (EV_BATCH_COLOUR for the colour-producing network: c->dominant and with it nerf_kernel_time_query
    // belong to image renders)
    j.kind_colour = EV_BATCH_COLOUR; j.what = "batch"; j.st = q.st;
    const bool with_normals = q.want_normals || (q.points && q.h > 0.0f); // a points render with h > 0 makes its normals in the surface workspace
    j.batch = &q; j.h = q.h;
    j.certify = cert != nullptr;
    // per-ray bounds: a finite far below every t -- the certify kernels' interval behind the last sample is clamped to 0 (cert_pass)
    j.far_cert = q.bounds ? -3.0e38f : q.far_;
    size_t pass_cap = pass_capacity(c, j.M);
    // normals: if every sample of a pass were live its 6 stencil points each must still fit one MLP launch
    if (with_normals) pass_cap = std::max<size_t>(1, std::min<size_t>(pass_cap, max_batch_points(c->n_cus) / (6 * (size_t)j.M)));
    j.n_rays = q.n_rays; j.pass_rays = std::min(q.n_rays, pass_cap);
    if ((rc = ensure_workspace(c, j.pass_rays, j.nc, j.M, j.coarse_only))) return rc;
    j.n_comp = j.coarse_only ? j.nc : j.M;
    const size_t n_comp_max = j.pass_rays * (size_t)j.n_comp;
    if (with_normals && (rc = c->buf[BUF_NORMAL].ensure(c, NormalWorkspace(nullptr, j.pass_rays, n_comp_max).bytes))) return rc;
    j.nw = NormalWorkspace(c->buf[BUF_NORMAL].p, j.pass_rays, n_comp_max);
    c->normal_live = 0; c->normal_samples = 0;
    j.normals = q.want_normals ? q.normals : nullptr;
    // quantile depths and points: the weights are the normals workspace's when there is one; a points render composites over black into the
    // surface workspace (colour C, opacity A per ray of the batch) and compacts from there
    SurfaceWorkspace sw;
    if (q.want_quantiles || q.points) {
        const size_t w_samples = with_normals ? 0 : n_comp_max, batch_rays = q.points ? q.n_rays : 0;
        if ((rc = c->buf[BUF_SURFACE].ensure(c, SurfaceWorkspace(nullptr, w_samples, j.pass_rays, batch_rays, with_normals).bytes))) return rc;
        sw = SurfaceWorkspace(c->buf[BUF_SURFACE].p, w_samples, j.pass_rays, batch_rays, with_normals);
        j.w_surface = with_normals ? j.nw.w : sw.w;
        j.n_q = q.points ? 1 : q.n_q;
        for (int k = 0; k < j.n_q; ++k) j.quant[k] = q.points ? q.quantile : q.quantiles[k];
        j.depth_q = q.points ? sw.depth_q : q.depth_q; j.depth_q_stride = q.n_rays;
    }
    if (q.points) {
        static const float kBlack[3] = {0.0f, 0.0f, 0.0f};
        j.background = kBlack; j.out = sw.rgb; j.depth = nullptr; j.opacity = sw.opacity;
        if (with_normals) j.normals = sw.normals;
        j.points = true;
        j.pg.min_opacity = q.min_opacity; j.pg.capacity = (uint32_t)std::min<size_t>(q.capacity, 0xffffffffu);
        j.pg.bsum = sw.bsum; j.pg.ray_of = sw.ray_of; j.pg.state = sw.state;
        j.pg.xyz_out = q.p_xyz; j.pg.rgb_out = q.p_rgb; j.pg.normals_out = with_normals ? q.p_normals : nullptr;
        j.pg.ray_out = q.p_ray; j.pg.depth_out = q.p_depth; j.pg.opacity_out = q.p_opacity;
        HIP_TRY(c, hipMemsetAsync(sw.state, 0, sizeof(PointState), q.st));
    }
    // BUF_BATCH (floats): [far per ray, padded to 64][points 3 x n SoA][directions n x 3 AoS], n = the pass's rays x M
    const bool expand = q.n_origins != 1 && !j.certify;
    const size_t far_floats = q.bounds ? (j.pass_rays + 63) / 64 * 64 : 0, n_max = j.pass_rays * (size_t)j.M;
    if (far_floats || expand) {
        if ((rc = c->buf[BUF_BATCH].ensure(c, (far_floats + (expand ? 6 * n_max : 0)) * sizeof(float)))) return rc;
        j.d_far = q.bounds ? c->dev(BUF_BATCH) : nullptr;
        j.d_pts = c->dev(BUF_BATCH) + far_floats; j.d_daos = j.d_pts + 3 * n_max;
    }
    if (q.h_origin) copy3(j.origin, q.h_origin);
    if (j.certify && (rc = reserve_certify(c, j, (j.n_rays + j.pass_rays - 1) / j.pass_rays, cert))) return rc;
    recycle_render(c);
    uint32_t passes = 0;
    if ((rc = render_passes(c, j, &passes))) return rc;
    if (j.points) HIP_TRY(c, launch_point_total(sw.state, q.d_n_points, q.st));
    if (cert && (rc = read_cert_outcome(c, j, passes, cert))) return rc;
    if ((rc = finish_stats(c, j, passes, q.stats, cert))) return rc;
    if (j.points && (q.n_points || q.stats)) { // the count on the host: 16 bytes and one stream synchronisation
        PointState hs{};
        HIP_TRY(c, hipMemcpyAsync(&hs, sw.state, sizeof hs, hipMemcpyDeviceToHost, q.st));
        HIP_TRY(c, hipStreamSynchronize(q.st));
        if (q.n_points) *q.n_points = hs.running;
        if ((size_t)hs.running > q.capacity) {
            char msg[160];
            snprintf(msg, sizeof msg, "point cloud: %u rays are kept but the capacity is %zu points; the first %zu are written", hs.running, q.capacity, q.capacity);
            return fail(c, NERF_ERR_STATE, msg);
        }
    }
    return NERF_OK;
}

// everything nerf_render_rays* can refuse without a context or a device, in the header's order
// q.certified: the nerf_render_rays*_certified forms -- the entry point is the switch, opts->certify_zero is only checked for its range
int check_ray_batch(nerf_ctx *c, const RayRequest &q) {
    const nerf_render_opts *o = q.opts;
    if (!o) return fail(c, NERF_ERR_INVALID, "opts is NULL");
    if (q.n_rays > (size_t)0x7fffffff) return fail(c, NERF_ERR_INVALID, "n_rays must be at most INT32_MAX");
    if (q.n_rays > 0 && (!q.origins || !q.dirs || !q.rgb)) return fail(c, NERF_ERR_INVALID, "origins, dirs and rgb_out must not be NULL");
    if (q.n_origins != 1 && q.n_origins != q.n_rays) return fail(c, NERF_ERR_INVALID, "n_origins must be 1 (one origin for every ray) or n_rays");
    if (o->crop_x0 || o->crop_y0 || o->crop_w || o->crop_h) return fail(c, NERF_ERR_INVALID, "ray batches have no pixel grid: crop_* must be 0");
    if (o->ssaa > 1) return fail(c, NERF_ERR_INVALID, "ray batches have no pixel grid: ssaa must be 0 or 1");
    if (o->band_count > 1) return fail(c, NERF_ERR_INVALID, "ray batches have no rows: band_count must be 0 or 1");
    if (o->skip_empty || o->skip_dead || o->hybrid_sampling || (o->certify_zero && !q.certified))
        return fail(c, NERF_ERR_INVALID, "skip_empty, skip_dead, hybrid_sampling and certify_zero are not available for ray batches (first version)");
    if (o->certify_zero != 0 && o->certify_zero != 1) return fail(c, NERF_ERR_INVALID, "certify_zero must be 0 or 1");
    int rc;
    if ((rc = check_sample_plan(c, o, PLAN_COUNTS))) return rc;
    if (q.certified && o->mlp_dtype == NERF_MLP_BF16) // the image path's refusal (check_image_modes)
        return fail(c, NERF_ERR_INVALID, "certify_zero needs mlp_dtype F32, BF16X3 or F16X2 and neither skip_empty nor skip_dead");
    if (!q.bounds) {
        if (!std::isfinite(q.near_) || !std::isfinite(q.far_)) return fail(c, NERF_ERR_INVALID, "near_ and far_ must be finite when bounds is NULL");
        if (!(q.far_ > q.near_)) return fail(c, NERF_ERR_INVALID, "far_ must be greater than near_ when bounds is NULL");
    }
    if (q.background && !(std::isfinite(q.background[0]) && std::isfinite(q.background[1]) && std::isfinite(q.background[2])))
        return fail(c, NERF_ERR_INVALID, "background components must be finite");
    return check_sample_plan(c, o, PLAN_LIMITS);
}

// the host entry points' per-ray checks: the first offending ray is named
int check_ray_batch_rays(nerf_ctx *c, const RayRequest &q) {
    char msg[160];
    auto finite3 = [](const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    for (size_t r = 0; r < q.n_rays; ++r) {
        const char *what = nullptr;
        const float *d = q.dirs + 3 * r, *b = q.bounds ? q.bounds + 2 * r : nullptr;
        if (r < q.n_origins && !finite3(q.origins + 3 * r)) what = "its origin is not finite";
        else if (!finite3(d)) what = "its direction is not finite";
        else if (q.normalize && d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) what = "its direction is zero and cannot be normalised";
        else if (b && !(std::isfinite(b[0]) && std::isfinite(b[1]))) what = "its bounds are not finite";
        else if (b && !(b[1] > b[0])) what = "its far is not greater than its near";
        if (what) {
            snprintf(msg, sizeof msg, "ray %zu: %s", r, what);
            return fail(c, NERF_ERR_INVALID, msg);
        }
    }
    return NERF_OK;
}

// what nerf_render_rays_normals* adds to check_ray_batch
int check_normals(nerf_ctx *c, const RayRequest &q) {
    if (!(std::isfinite(q.h) && q.h > 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and greater than 0");
    if (!q.normals) return fail(c, NERF_ERR_INVALID, "normals_out must not be NULL");
    return NERF_OK;
}

// what nerf_render_rays_quantiles* and nerf_render_rays_points* add to check_ray_batch, in the header's order
int check_surface(nerf_ctx *c, const RayRequest &q) {
    auto quantile_ok = [](float v) { return std::isfinite(v) && v > 0.0f && v <= 1.0f; };
    if (q.want_quantiles) {
        if (q.n_q < 1 || q.n_q > NERF_MAX_QUANTILES) return fail(c, NERF_ERR_INVALID, "n_q must be between 1 and NERF_MAX_QUANTILES (8)");
        if (!q.quantiles) return fail(c, NERF_ERR_INVALID, "quantiles must not be NULL");
        for (int k = 0; k < q.n_q; ++k)
            if (!quantile_ok(q.quantiles[k])) return fail(c, NERF_ERR_INVALID, "a quantile must be finite and lie in (0, 1]");
        if (q.n_rays > 0 && !q.depth_q) return fail(c, NERF_ERR_INVALID, "depth_q_out must not be NULL");
        return NERF_OK;
    }
    if (!quantile_ok(q.quantile)) return fail(c, NERF_ERR_INVALID, "a quantile must be finite and lie in (0, 1]");
    if (!(std::isfinite(q.min_opacity) && q.min_opacity >= 0.0f && q.min_opacity <= 1.0f)) return fail(c, NERF_ERR_INVALID, "min_opacity must be finite and lie in [0, 1]");
    if (!(std::isfinite(q.h) && q.h >= 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and not negative");
    if (q.n_rays > 0 && q.capacity > 0 && !q.p_xyz) return fail(c, NERF_ERR_INVALID, "xyz_out must not be NULL");
    if (q.p_normals && !(q.h > 0.0f)) return fail(c, NERF_ERR_INVALID, "normals_out needs h > 0");
    if (q.h > 0.0f && !q.p_normals) return fail(c, NERF_ERR_INVALID, "h > 0 needs normals_out");
    return NERF_OK;
}

// what nerf_render_rays_clipped* refuses without a context or a device: nerf_render_rays' refusals, then the grid's
int check_rays_clipped(nerf_ctx *c, const RayRequest &q) {
    int rc;
    if ((rc = check_ray_batch(c, q))) return rc;
    if (const char *why = nerfclip::check_grid(q.occ_bits, q.lo, q.step, q.dims)) return fail(c, NERF_ERR_INVALID, why);
    return NERF_OK;
}

// Everything one of the fourteen entry points refuses before it touches the device, in the header's order; host: the arrays are host memory,
// so their rays are checked one by one.  "ctx is NULL" comes last, and *n_hit is cleared behind it (before the n_rays == 0 return).
int check_request(nerf_ctx *c, const RayRequest &q, bool host) {
    int rc;
    if ((rc = q.clipped ? check_rays_clipped(c, q) : check_ray_batch(c, q))) return rc;
    if (q.want_normals && (rc = check_normals(c, q))) return rc;
    if ((q.want_quantiles || q.points) && (rc = check_surface(c, q))) return rc;
    if (host && (rc = check_ray_batch_rays(c, q))) return rc;
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (q.clipped && q.n_hit) *q.n_hit = 0;
    if (q.points && q.n_points) *q.n_points = 0;
    return NERF_OK;
}

// certify_zero renders are AUDITED (k_cert_audit: 1 in 16 of the samples certified by less than twice the margin and 1 in 128 of the others are evaluated exactly all the same).  A frame stands only if no
// audited certificate was wrong and the closest audited sample kept at least half the margin between itself and a positive density;
// otherwise the network's margin is widened -- for good: c->cert_margin is per context and network, reset when a network is loaded --
// and the frame is rendered again.  The same loop grows the sample list when a pass wanted more entries than it had.  Margins are
// measurements, not proofs: what this buys is that a network on which bf16 is less accurate than on the lego scene
// calibrates itself or fails loudly (NERF_ERR_STATE) instead of returning a silently different frame.
// Every attempt writes the whole frame -- colour and the requested maps -- so the maps returned are those of the frame that stands.
// One copy for image renders (render_device) and certified ray batches (run_rays): attempt(&outcome)
// renders the whole frame / batch once; what = "frame" / "batch".
template <class Attempt>
int certify_retry(nerf_ctx *c, nerf_stats *stats, const char *what, Attempt attempt) {
    constexpr int kMaxRetries = 8;
    uint64_t violations = 0;
    for (int tries = 0;; ++tries) {
        CertOutcome oc;
        const int rc = attempt(&oc);
        if (rc) return rc;
        bool again = false;
        std::string why;
        if (oc.list_need > oc.list_capacity) { // (entries beyond the capacity were counted, not stored)
            c->cert_list_frac = std::min(1.0, 1.25 * (double)oc.list_need / (double)std::max<uint64_t>(oc.pass_samples, 1));
            again = true;
            why = "the sample list was too short";
        }
        for (int w = 0; w < 2; ++w)
            if (oc.range_left[w]) { // the f16 pre-filter met an activation beyond 65 504: its pre-activations are void -- bf16 (f32's range) from now on
                c->cert_prefilter_f16[w] = false;
                c->cert_margin[w] = std::max(c->cert_margin[w], c->cert_margin_floor[w]);
                again = true;
                why = "an activation left the range of the f16 pre-filter";
            }
        const bool overflow = again; // an attempt whose list was too short evaluated only a part of it (or whose pre-filter left its range): its audit says nothing
        if (!overflow) violations += oc.violations[0] + oc.violations[1];
        for (int w = 0; w < 2 && !overflow; ++w) {
            if (!oc.used[w] || !oc.audited[w]) continue;
            // the rules live in host_util.cpp (certify_policy: tested on the CPU through nerf_debug_certify_policy)
            float widened = c->cert_margin[w];
            const int rule = certify_policy(c->cert_margin[w], oc.audited[w], oc.violations[w], oc.headroom[w], oc.max_err[w], &widened);
            if (rule) {
                c->cert_margin[w] = widened; again = true;
                why = rule == 1 ? "an audited certificate was wrong" : rule == 2 ? "an audited certificate came closer to a positive density than half the margin"
                                                                                 : "the 16-bit pass was off by more than half the margin on an audited certificate";
            }
        }
        if (stats) { stats->n_certify_retries = (uint32_t)tries; stats->n_certify_violations = violations; }
        if (!again) return NERF_OK;
        if (tries == kMaxRetries) {
            char msg[320];
            snprintf(msg, sizeof msg, "certify_zero: %s after %d renders of this %s (margins now %g / %g): the 16-bit pass cannot certify this network's "
                     "zero densities; render with certify_zero = 0", why.c_str(), tries + 1, what, (double)c->cert_margin[0], (double)c->cert_margin[1]);
            return fail(c, NERF_ERR_STATE, msg);
        }
    }
}

} // namespace

int nerfint::render_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, float *d_out, float *d_depth, float *d_opacity,
                           hipStream_t st, nerf_stats *stats, const float *background) {
    if (!o || !o->certify_zero) return render_once(c, cam, o, d_out, d_depth, d_opacity, st, stats, nullptr, background);
    return certify_retry(c, stats, "frame", [&](CertOutcome *oc) { return render_once(c, cam, o, d_out, d_depth, d_opacity, st, stats, oc, background); });
}

int nerfint::output_window(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, size_t *w_out, size_t *h_out) {
    int rc;
    if ((rc = check_camera(c, cam))) return rc;
    if (!opts) return fail(c, NERF_ERR_INVALID, "opts is NULL");
    const bool crop = opts->crop_w > 0 || opts->crop_h > 0;
    const long long w = crop ? opts->crop_w : cam->nx;
    long long h = crop ? opts->crop_h : cam->ny;
    if (w <= 0 || h <= 0) return fail(c, NERF_ERR_INVALID, "crop window outside the frame");
    if (opts->band_count > 1) {
        if (opts->band_index < 0 || opts->band_index >= opts->band_count || opts->band_stripe_rows < 0) return fail(c, NERF_ERR_INVALID, "band_index / band_count / band_stripe_rows out of range");
        h = band_rows((int)h, opts->band_index, opts->band_count, opts->band_stripe_rows);
        if (h <= 0) return fail(c, NERF_ERR_INVALID, "this band has no rows (more bands than rows)");
    }
    *w_out = (size_t)w; *h_out = (size_t)h;
    return NERF_OK;
}

static size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// The f32 frame (and the opacity plane of the two alpha modes) live in the context's own workspace, grown on demand: a warm call
// allocates nothing.  Conversion and quantisation run once per pixel, on the frame that stands (behind the box filter and behind
// certify_zero's retry loop, both inside render_device).
int nerfint::render_rgba8_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, const float *background, int alpha_mode,
                                 uint8_t *d_rgba, hipStream_t st, nerf_stats *stats) {
    int rc;
    const float *bg = nullptr;
    if ((rc = check_rgba8(c, background, alpha_mode, d_rgba, &bg))) return rc;
    size_t w = 0, h = 0;
    if ((rc = output_window(c, cam, o, &w, &h))) return rc;
    const size_t px = w * h, op_at = align4(3 * px);
    if ((rc = c->buf[BUF_PACK].ensure(c, (op_at + px) * sizeof(float)))) return rc;
    float *d_rgb = c->dev(BUF_PACK), *d_opacity = alpha_mode == NERF_ALPHA_OPAQUE ? nullptr : d_rgb + op_at;
    if ((rc = render_device(c, cam, o, d_rgb, nullptr, d_opacity, st, stats, bg))) return rc;
    HIP_TRY(c, launch_pack_rgba8(d_rgb, d_opacity, (uint32_t *)d_rgba, px, alpha_mode, st));
    if (stats) HIP_TRY(c, hipStreamSynchronize(st)); // as the float variant: with stats the output is complete on return
    return NERF_OK;
}

extern "C" {

int nerf_render_image_aux_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, float *d_rgb_out,
                                 float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    DeviceGuard dg(c->device);
    return render_device(c, cam, opts, d_rgb_out, d_depth_out, d_opacity_out, (hipStream_t)stream, stats);
} NERF_CATCH(c)

int nerf_render_image_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, float *d_rgb_out,
                             void *stream, nerf_stats *stats) {
    return nerf_render_image_aux_device(c, cam, opts, d_rgb_out, nullptr, nullptr, stream, stats);
}

int nerf_render_image_aux(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, float *rgb_out, float *depth_out,
                          float *opacity_out, nerf_stats *stats) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (!rgb_out) return fail(c, NERF_ERR_INVALID, "output pointer is NULL");
    int rc;
    size_t w = 0, h = 0;
    if ((rc = output_window(c, cam, opts, &w, &h))) return rc;
    DeviceGuard dg(c->device);
    // staging: the colour, then each requested map (w x h floats)
    const size_t px = w * h;
    Staging s(c, BUF_OUT, c->stream);
    const int i_rgb = s.add(sizeof(float), 3 * px, nullptr, rgb_out), i_depth = s.opt(depth_out, sizeof(float), px, nullptr, depth_out),
              i_opacity = s.opt(opacity_out, sizeof(float), px, nullptr, opacity_out);
    if ((rc = s.begin())) return rc;
    nerf_stats local; // a synchronous render always reads its counters: a frame computed outside a split arithmetic's range is an error
    if ((rc = render_device(c, cam, opts, s.at(i_rgb), s.at(i_depth), s.at(i_opacity), c->stream, stats ? stats : &local))) return rc;
    return s.finish();
} NERF_CATCH(c)

int nerf_render_image(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, float *rgb_out, nerf_stats *stats) {
    return nerf_render_image_aux(c, cam, opts, rgb_out, nullptr, nullptr, stats);
}

int nerf_render_image_rgba8_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, const float background[3], int alpha_mode,
                                   uint8_t *d_rgba_out, void *stream, nerf_stats *stats) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    DeviceGuard dg(c->device);
    return render_rgba8_device(c, cam, opts, background, alpha_mode, d_rgba_out, (hipStream_t)stream, stats);
} NERF_CATCH(c)

int nerf_render_image_rgba8(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *opts, const float background[3], int alpha_mode,
                            uint8_t *rgba_out, nerf_stats *stats) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    int rc;
    const float *bg = nullptr;
    if ((rc = check_rgba8(c, background, alpha_mode, rgba_out, &bg))) return rc;
    size_t w = 0, h = 0;
    if ((rc = output_window(c, cam, opts, &w, &h))) return rc;
    DeviceGuard dg(c->device);
    Staging s(c, BUF_OUT, c->stream); // 4 bytes per pixel come back instead of 12 (16 with the opacity)
    const int i_rgba = s.add(4, w * h, nullptr, rgba_out);
    if ((rc = s.begin())) return rc;
    nerf_stats local; // a synchronous render always reads its counters (see nerf_render_image_aux)
    if ((rc = render_rgba8_device(c, cam, opts, background, alpha_mode, s.at<uint8_t>(i_rgba), c->stream, stats ? stats : &local))) return rc;
    return s.finish();
} NERF_CATCH(c)

// ---- ray batches ---------------------------------------------------------------------------------------------------------------------
// one render of a device request whose shared origin (if any) is known on the host; a certified one goes through the retry loop, which
// renders the batch again
static int run_rays(nerf_ctx *c, const RayRequest &q) {
    if (!q.certified) return render_rays_device(c, q, nullptr);
    return certify_retry(c, q.stats, "batch", [&](CertOutcome *oc) { return render_rays_device(c, q, oc); });
}

// nerf_render_rays*_device without a grid
static int rays_device(nerf_ctx *c, RayRequest q) {
    float origin[3];
    if (q.n_origins == 1 && !q.h_origin) { // the shared origin rides in the MLP kernels' arguments: 12 bytes come back first
        HIP_TRY(c, hipMemcpyAsync(origin, q.origins, sizeof origin, hipMemcpyDeviceToHost, q.st));
        HIP_TRY(c, hipStreamSynchronize(q.st));
        q.h_origin = origin;
    }
    return run_rays(c, q);
}

// ---- clipped ray batches -----------------------------------------------------------------------------------------------------
// nerf_render_rays_clipped*_device: clip -> count -> [gather -> the compacted batch through run_rays -> scatter].  certified: the compacted
// batch is rendered with zero certification; a retry renders the compacted batch again and does not clip again
static int rays_clipped_device(nerf_ctx *c, const RayRequest &q) {
    int rc;
    const hipStream_t st = q.st;
    const bool per_ray = q.n_origins != 1;
    if ((rc = c->buf[BUF_CLIP].ensure(c, ClipWorkspace(nullptr, q.n_rays, per_ray).bytes))) return rc;
    const ClipWorkspace w(c->buf[BUF_CLIP].p, q.n_rays, per_ray);
    ClipRaysArgs a{};
    a.bits = q.occ_bits;
    for (int k = 0; k < 3; ++k) { a.lo[k] = q.lo[k]; a.step[k] = q.step[k]; a.dims[k] = q.dims[k]; a.bg[k] = q.background ? q.background[k] : 1.0f; }
    a.origins = q.origins; a.per_ray_origins = per_ray ? 1 : 0; a.dirs = q.dirs; a.n_rays = (int)q.n_rays; a.normalize = q.normalize ? 1 : 0;
    a.near_ = q.near_; a.far_ = q.far_; a.bounds = q.bounds; a.bounds_out = w.clip_bounds; a.hit_out = q.hit ? q.hit : w.hit; a.bsum = w.bsum;
    a.rgb_fill = q.rgb; a.depth_fill = q.depth; a.opacity_fill = q.opacity; // the missed rays are finished here
    HIP_TRY(c, launch_clip_rays(a, st));
    HIP_TRY(c, launch_clip_scan(w.bsum, a.n_rays, w.totals, st));
    uint32_t totals[2] = {0, 0};
    float origin[3] = {0.0f, 0.0f, 0.0f};
    HIP_TRY(c, hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, st));
    if (!per_ray) HIP_TRY(c, hipMemcpyAsync(origin, q.origins, sizeof origin, hipMemcpyDeviceToHost, st)); // rides in the MLP kernels' arguments
    HIP_TRY(c, hipStreamSynchronize(st)); // the hit count sizes every launch that follows
    const size_t H = totals[0];
    if (H > q.n_rays) return fail(c, NERF_ERR_HIP, "clipped render: the hit count exceeds the batch");
    if (q.n_hit) *q.n_hit = H;
    if (H == 0) { // nothing to render: the clip launch has written every ray
        if (q.stats) memset(q.stats, 0, sizeof *q.stats);
        return NERF_OK;
    }
    ClipGatherArgs g{};
    g.n_rays = a.n_rays; g.hit = a.hit_out; g.bsum = w.bsum; g.dirs = q.dirs; g.origins = per_ray ? q.origins : nullptr; g.clip_bounds = w.clip_bounds;
    g.rng_index = q.rng_index; g.ray_of = w.ray_of; g.dirs_c = w.dirs_c; g.origins_c = w.origins_c; g.bounds_c = w.bounds_c; g.rng_c = w.rng_c;
    HIP_TRY(c, launch_clip_gather(g, st));
    RayRequest b = q; // the compacted batch
    b.origins = per_ray ? w.origins_c : q.origins; b.n_origins = per_ray ? H : 1; b.h_origin = per_ray ? nullptr : origin;
    b.dirs = w.dirs_c; b.n_rays = H; b.bounds = w.bounds_c; b.rng_index = w.rng_c;
    b.rgb = w.rgb_c; b.depth = q.depth ? w.depth_c : nullptr; b.opacity = q.opacity ? w.opacity_c : nullptr;
    if ((rc = run_rays(c, b))) return rc;
    const ClipScatterArgs s{(uint32_t)H, w.ray_of, w.rgb_c, w.depth_c, w.opacity_c, q.rgb, q.depth, q.opacity};
    HIP_TRY(c, launch_clip_scatter(s, st));
    if (q.stats || q.certified) HIP_TRY(c, hipStreamSynchronize(st)); // as nerf_render_rays_device: with stats the outputs are complete on return; certified forms always are
    return NERF_OK;
}

// nerf_render_rays_points on host arrays: the rays go up, the device form runs, and of every output array the records that were written --
// the first min(count, capacity) -- come down; the caller's arrays behind them stay untouched.
static int points_host(nerf_ctx *c, const RayRequest &q) {
    int rc;
    const size_t R = q.n_rays, F = sizeof(float), cap = std::min(q.capacity, R); // a batch keeps at most n_rays points
    const bool up_origins = q.n_origins != 1;
    Staging s(c, BUF_OUT, c->stream);
    const int i_dirs = s.add(F, 3 * R, q.dirs), i_origins = s.opt(up_origins, F, 3 * q.n_origins, q.origins), i_bounds = s.opt(q.bounds, F, 2 * R, q.bounds),
              i_rng = s.opt(q.rng_index, sizeof(uint32_t), R, q.rng_index), i_xyz = s.add(F, 3 * cap), i_rgb = s.add(F, 3 * cap),
              i_nrm = s.opt(q.p_normals, F, 3 * cap), i_ray = s.opt(q.p_ray, sizeof(uint32_t), cap), i_depth = s.opt(q.p_depth, F, cap),
              i_opacity = s.opt(q.p_opacity, F, cap);
    if ((rc = s.begin())) return rc;
    nerf_stats local; // a synchronous render always reads its counters (see nerf_render_image_aux)
    size_t count = 0;
    RayRequest d = q;
    d.dirs = s.at(i_dirs); d.origins = s.at(i_origins); d.bounds = s.at(i_bounds); d.rng_index = s.at<uint32_t>(i_rng);
    d.p_xyz = s.at(i_xyz); d.p_rgb = s.at(i_rgb); d.p_normals = s.at(i_nrm); d.p_ray = s.at<uint32_t>(i_ray); d.p_depth = s.at(i_depth);
    d.p_opacity = s.at(i_opacity); d.capacity = cap; d.n_points = &count; d.d_n_points = nullptr;
    d.h_origin = up_origins ? nullptr : q.origins;
    d.st = c->stream; d.stats = q.stats ? q.stats : &local;
    rc = rays_device(c, d);
    if (rc && rc != NERF_ERR_STATE) return rc; // NERF_ERR_STATE with a count: more rays are kept than fit, the first `capacity` points stand
    if (q.n_points) *q.n_points = count;
    const size_t m = std::min(count, cap);
    if (m > 0) {
        HIP_TRY(c, hipMemcpyAsync(q.p_xyz, d.p_xyz, 3 * m * F, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(q.p_rgb, d.p_rgb, 3 * m * F, hipMemcpyDeviceToHost, c->stream));
        if (q.p_normals) HIP_TRY(c, hipMemcpyAsync(q.p_normals, d.p_normals, 3 * m * F, hipMemcpyDeviceToHost, c->stream));
        if (q.p_ray) HIP_TRY(c, hipMemcpyAsync(q.p_ray, d.p_ray, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (q.p_depth) HIP_TRY(c, hipMemcpyAsync(q.p_depth, d.p_depth, m * F, hipMemcpyDeviceToHost, c->stream));
        if (q.p_opacity) HIP_TRY(c, hipMemcpyAsync(q.p_opacity, d.p_opacity, m * F, hipMemcpyDeviceToHost, c->stream));
    }
    const std::string why = rc ? c->err : std::string();
    const int rc2 = s.finish();
    return rc2 ? rc2 : rc ? fail(c, rc, why) : NERF_OK;
}

// The fourteen entry points: refuse, [stage the host arrays], run the device form, [download].  host: every array of q is host memory.
static int render_rays_entry(nerf_ctx *c, const RayRequest &q, bool host) {
    int rc;
    if ((rc = check_request(c, q, host))) return rc;
    if (q.n_rays == 0) { // a no-op; only an empty point cloud with a device count has something to write
        if (q.points && q.d_n_points) {
            DeviceGuard dg(c->device);
            HIP_TRY(c, hipMemsetAsync(q.d_n_points, 0, sizeof(uint32_t), q.st));
        }
        return NERF_OK;
    }
    DeviceGuard dg(c->device);
    if (!host) return q.clipped ? rays_clipped_device(c, q) : rays_device(c, q);
    if (q.points) return points_host(c, q);
    // staging: [occupancy], dirs, [origins], [bounds], [rng_index], rgb, [depth], [opacity], [normals], [hit flags].  One origin for every
    // ray stays on the host (h_origin) unless the clip launch reads it
    const size_t R = q.n_rays, F = sizeof(float);
    const bool up_origins = q.clipped || q.n_origins != 1;
    Staging s(c, BUF_OUT, c->stream);
    const int i_occ = s.opt(q.clipped, sizeof(uint32_t), q.clipped ? ((size_t)q.dims[0] * q.dims[1] * q.dims[2] + 31) / 32 : 0, q.occ_bits),
              i_dirs = s.add(F, 3 * R, q.dirs), i_origins = s.opt(up_origins, F, 3 * q.n_origins, q.origins), i_bounds = s.opt(q.bounds, F, 2 * R, q.bounds),
              i_rng = s.opt(q.rng_index, sizeof(uint32_t), R, q.rng_index), i_rgb = s.add(F, 3 * R, nullptr, q.rgb),
              i_depth = s.opt(q.depth, F, R, nullptr, q.depth), i_opacity = s.opt(q.opacity, F, R, nullptr, q.opacity),
              i_normals = s.opt(q.want_normals, F, 3 * R, nullptr, q.normals), i_hit = s.opt(q.clipped && q.hit, 1, R, nullptr, q.hit),
              i_dq = s.opt(q.want_quantiles, F, (size_t)(q.want_quantiles ? q.n_q : 0) * R, nullptr, q.depth_q);
    if ((rc = s.begin())) return rc;
    nerf_stats local; // a synchronous render always reads its counters (see nerf_render_image_aux)
    RayRequest d = q;
    d.occ_bits = s.at<uint32_t>(i_occ); d.dirs = s.at(i_dirs); d.origins = s.at(i_origins); d.bounds = s.at(i_bounds); d.rng_index = s.at<uint32_t>(i_rng);
    d.rgb = s.at(i_rgb); d.depth = s.at(i_depth); d.opacity = s.at(i_opacity); d.normals = s.at(i_normals); d.hit = s.at<uint8_t>(i_hit);
    d.depth_q = s.at(i_dq);
    d.h_origin = up_origins ? nullptr : q.origins;
    d.st = c->stream; d.stats = q.stats ? q.stats : &local;
    if ((rc = q.clipped ? rays_clipped_device(c, d) : rays_device(c, d))) return rc;
    return s.finish();
}

int nerf_render_rays(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_,
                     const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3], float *rgb_out,
                     float *depth_out, float *opacity_out, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out; q.opacity = opacity_out;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_,
                            float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts, const float background[3],
                            float *d_rgb_out, float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out; q.depth = d_depth_out;
    q.opacity = d_opacity_out; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

int nerf_render_rays_normals(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                             float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3],
                             float *rgb_out, float *depth_out, float *opacity_out, float h, float *normals_out, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out; q.opacity = opacity_out;
    q.want_normals = true; q.h = h; q.normals = normals_out;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_normals_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                    float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                    const float background[3], float *d_rgb_out, float *d_depth_out, float *d_opacity_out, float h,
                                    float *d_normals_out, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out; q.depth = d_depth_out;
    q.opacity = d_opacity_out; q.want_normals = true; q.h = h; q.normals = d_normals_out; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

int nerf_render_rays_certified(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                               float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3],
                               float *rgb_out, float *depth_out, float *opacity_out, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out; q.opacity = opacity_out;
    q.certified = true;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_certified_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                      float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                      const float background[3], float *d_rgb_out, float *d_depth_out, float *d_opacity_out, void *stream,
                                      nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out; q.depth = d_depth_out;
    q.opacity = d_opacity_out; q.certified = true; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

// quantile depths: `quantiles` is host memory in both forms
int nerf_render_rays_quantiles(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                               float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3],
                               float *rgb_out, float *depth_out, float *opacity_out, const float *quantiles, int n_q, float *depth_q_out,
                               nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out; q.opacity = opacity_out;
    q.want_quantiles = true; q.quantiles = quantiles; q.n_q = n_q; q.depth_q = depth_q_out;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_quantiles_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                      float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                      const float background[3], float *d_rgb_out, float *d_depth_out, float *d_opacity_out, const float *quantiles,
                                      int n_q, float *d_depth_q_out, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out; q.depth = d_depth_out;
    q.opacity = d_opacity_out; q.want_quantiles = true; q.quantiles = quantiles; q.n_q = n_q; q.depth_q = d_depth_q_out; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

// point clouds: q.rgb is the points' colour array, so that nerf_render_rays' "rgb_out must not be NULL" covers it
int nerf_render_rays_points(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                            float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, float quantile,
                            float min_opacity, float h, size_t capacity, float *xyz_out, float *rgb_out, float *normals_out, uint32_t *ray_out,
                            float *depth_out, float *opacity_out, size_t *n_points, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts;
    q.stats = stats;
    q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out;
    q.points = true; q.quantile = quantile; q.min_opacity = min_opacity; q.h = h; q.capacity = capacity;
    q.p_xyz = xyz_out; q.p_rgb = rgb_out; q.p_normals = normals_out; q.p_ray = ray_out; q.p_depth = depth_out; q.p_opacity = opacity_out;
    q.n_points = n_points;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_points_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                   float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                   float quantile, float min_opacity, float h, size_t capacity, float *d_xyz_out, float *d_rgb_out,
                                   float *d_normals_out, uint32_t *d_ray_out, float *d_depth_out, float *d_opacity_out, size_t *n_points,
                                   uint32_t *d_n_points, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts;
    q.stats = stats;
    q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out;
    q.points = true; q.quantile = quantile; q.min_opacity = min_opacity; q.h = h; q.capacity = capacity;
    q.p_xyz = d_xyz_out; q.p_rgb = d_rgb_out; q.p_normals = d_normals_out; q.p_ray = d_ray_out; q.p_depth = d_depth_out; q.p_opacity = d_opacity_out;
    q.n_points = n_points; q.d_n_points = d_n_points; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

// the four clipped forms: the grid, the flags and the hit count on top
int nerf_render_rays_clipped(nerf_ctx *c, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                             const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_,
                             const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3], float *rgb_out,
                             float *depth_out, float *opacity_out, uint8_t *hit_out, uint64_t *n_hit, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.clipped = true; q.lo = lo; q.step = step; q.dims = dims; q.n_hit = n_hit;
    q.occ_bits = occ_bits; q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out;
    q.opacity = opacity_out; q.hit = hit_out;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_clipped_device(nerf_ctx *c, const uint32_t *d_occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                                    const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_,
                                    float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                    const float background[3], float *d_rgb_out, float *d_depth_out, float *d_opacity_out, uint8_t *d_hit_out,
                                    uint64_t *n_hit, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.clipped = true; q.lo = lo; q.step = step; q.dims = dims; q.n_hit = n_hit;
    q.occ_bits = d_occ_bits; q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out;
    q.depth = d_depth_out; q.opacity = d_opacity_out; q.hit = d_hit_out; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

int nerf_render_rays_clipped_certified(nerf_ctx *c, const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                                       const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                                       float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts,
                                       const float background[3], float *rgb_out, float *depth_out, float *opacity_out, uint8_t *hit_out,
                                       uint64_t *n_hit, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.clipped = true; q.lo = lo; q.step = step; q.dims = dims; q.n_hit = n_hit;
    q.occ_bits = occ_bits; q.origins = origins; q.dirs = dirs; q.bounds = bounds; q.rng_index = rng_index; q.rgb = rgb_out; q.depth = depth_out;
    q.opacity = opacity_out; q.hit = hit_out; q.certified = true;
    return render_rays_entry(c, q, true);
} NERF_CATCH(c)

int nerf_render_rays_clipped_certified_device(nerf_ctx *c, const uint32_t *d_occ_bits, const float lo[3], const float step[3], const int32_t dims[3],
                                              const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                              float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index,
                                              const nerf_render_opts *opts, const float background[3], float *d_rgb_out, float *d_depth_out,
                                              float *d_opacity_out, uint8_t *d_hit_out, uint64_t *n_hit, void *stream, nerf_stats *stats) try {
    RayRequest q{};
    q.n_origins = n_origins; q.n_rays = n_rays; q.normalize = normalize; q.near_ = near_; q.far_ = far_; q.opts = opts; q.background = background;
    q.stats = stats;
    q.clipped = true; q.lo = lo; q.step = step; q.dims = dims; q.n_hit = n_hit;
    q.occ_bits = d_occ_bits; q.origins = d_origins; q.dirs = d_dirs; q.bounds = d_bounds; q.rng_index = d_rng_index; q.rgb = d_rgb_out;
    q.depth = d_depth_out; q.opacity = d_opacity_out; q.hit = d_hit_out; q.certified = true; q.st = (hipStream_t)stream;
    return render_rays_entry(c, q, false);
} NERF_CATCH(c)

} // extern "C"
