// nerf_context.cpp -- the context: creation and destruction, device memory that grows on demand, the event pool behind the kernel timings,
// and the entry points that only read the context (include/nerf_mi355x.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <set>

#include "../../include/nerf_mi355x.h"
#include "host_util.h"
#include "mlp_kernel.h"
#include "sampling_kernels.h"

#include "nerf_internal.h"

namespace nerfint {

int fail(nerf_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return nerfhost::fail_noctx(code, msg); // also recorded for nerf_last_error(NULL) of this thread
}

hipEvent_t get_event(nerf_ctx *c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void recycle_render(nerf_ctx *c) {
    for (auto &p : c->last_render) if (!p.dominant) { c->ev_pool.push_back(p.a); c->ev_pool.push_back(p.b); }
    c->last_render.clear();
}

void recycle_dominant(nerf_ctx *c, size_t keep) {
    while (c->dominant.size() > keep) {
        c->ev_pool.push_back(c->dominant.front().a); c->ev_pool.push_back(c->dominant.front().b);
        c->dominant.erase(c->dominant.begin());
    }
}

int DevBuf::ensure(nerf_ctx *c, size_t need) {
    if (bytes >= need) return NERF_OK;
    if (p) { HIP_TRY(c, hipDeviceSynchronize()); HIP_TRY(c, hipFree(p)); p = nullptr; bytes = 0; }
    HIP_TRY(c, hipMalloc(&p, need));
    bytes = need;
    return NERF_OK;
}

int DevBuf::release(nerf_ctx *c) {
    if (!p) return NERF_OK;
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipFree(p));
    p = nullptr; bytes = 0;
    return NERF_OK;
}

int Staging::begin() {
    if (refused) return fail(c, NERF_ERR_INVALID, "internal error: staging layout too large");
    int rc;
    if ((rc = buf.ensure(c, total))) return rc;
    for (int k = 0; k < n_parts; ++k) {
        const Part &q = parts[k];
        if (!q.bytes) continue;
        if (q.upload) HIP_TRY(c, hipMemcpyAsync(at<char>(k), q.upload, q.bytes, hipMemcpyHostToDevice, st));
        if (q.fill != kNoFill) HIP_TRY(c, hipMemsetAsync(at<char>(k), q.fill, q.bytes, st));
    }
    return NERF_OK;
}

int Staging::finish() {
    for (int k = 0; k < n_parts; ++k)
        if (parts[k].download && parts[k].bytes) HIP_TRY(c, hipMemcpyAsync(parts[k].download, at<char>(k), parts[k].bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return NERF_OK;
}

// The coarse network's colours exist only in a coarse_only render (the reference discards them otherwise, src/lib.rs:404):
// their buffer (rays x nc x 3 floats, 492 MB for an 800x800 pass) is allocated on first such use only.
int ensure_workspace(nerf_ctx *c, size_t rays, size_t nc, size_t m, bool need_rgbc) {
    if (rays <= c->ws_rays && nc <= c->ws_nc && m <= c->ws_m && (!need_rgbc || c->buf[BUF_RGBC].p)) return NERF_OK;
    rays = std::max(rays, c->ws_rays); nc = std::max(nc, c->ws_nc); m = std::max(m, c->ws_m);
    need_rgbc = need_rgbc || c->buf[BUF_RGBC].p != nullptr;
    HIP_TRY(c, hipDeviceSynchronize());
    for (int k = BUF_DIRS; k <= BUF_RGBF; ++k) {
        DevBuf &b = c->buf[k];
        if (b.p) { HIP_TRY(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    }
    c->ws_rays = c->ws_nc = c->ws_m = 0;
    const size_t floats[] = {rays * 3, rays * nc, rays * nc, need_rgbc ? rays * nc * 3 : 0, rays * m, rays * m, rays * m * 3};
    for (int k = BUF_DIRS; k <= BUF_RGBF; ++k) {
        DevBuf &b = c->buf[k];
        if (k == BUF_RGBC && !need_rgbc) continue;
        HIP_TRY(c, hipMalloc(&b.p, floats[k - BUF_DIRS] * sizeof(float)));
        b.bytes = floats[k - BUF_DIRS] * sizeof(float);
    }
    c->ws_rays = rays; c->ws_nc = nc; c->ws_m = m;
    return NERF_OK;
}

} // namespace nerfint

using namespace nerfint;

// a size from the environment: kept as it is unless the variable holds a positive integer
static void env_size(const char *name, size_t *out) {
    const char *env = getenv(name);
    if (env && atoll(env) > 0) *out = (size_t)atoll(env);
}

extern "C" {

int nerf_abi_version(void) { return 5; }

void nerf_abi_struct_sizes(size_t *camera, size_t *render_opts, size_t *stats) {
    if (camera) *camera = sizeof(nerf_camera);
    if (render_opts) *render_opts = sizeof(nerf_render_opts);
    if (stats) *stats = sizeof(nerf_stats);
}

const char *nerf_last_error(const nerf_ctx *ctx) { return ctx ? ctx->err.c_str() : nerfhost::last_error_noctx(); }

int nerf_create(int device_id, nerf_ctx **out) try {
    if (!out) return fail(nullptr, NERF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, NERF_ERR_HIP, std::string("no HIP device available (") + hipGetErrorString(e) + "); libnerf_mi355x has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(nullptr, NERF_ERR_INVALID, "device_id out of range");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    std::string arch = prop.gcnArchName;
    if (arch.rfind("gfx950", 0) != 0)
        return fail(nullptr, NERF_ERR_HIP, "device is " + arch + ", this library is built for gfx950 (MI355X) only");
    nerf_ctx *c = new nerf_ctx();
    c->device = device_id;
    c->n_cus = prop.multiProcessorCount;
    c->arch = arch;
    env_size("NERF_MAX_RAYS_PER_PASS", &c->max_rays_per_pass);
    env_size("NERF_MAX_EXPORT_BYTES", &c->max_export_bytes);
    if (const char *env = getenv("NERF_HYBRID_TAU")) { // experiments only: the predicted sample displacement (in t) above which a ray is redone in f32
        const double v = atof(env);
        if (v >= 0.0 && v <= 1.0) c->hybrid_tau = (float)v;
    }
#ifdef NERF_CERT_TUNING // variant builds only (make variant DEFS=-DNERF_CERT_TUNING=1): the product's certificates are not configurable from the environment
    if (const char *env = getenv("NERF_CERTIFY_SEQ_PREFILTER")) c->cert_seq_prefilter = atoi(env) != 0;
    if (const char *env = getenv("NERF_CERTIFY_PREFILTER_F16")) c->cert_allow_f16 = atoi(env) != 0;
    if (const char *env = getenv("NERF_CERTIFY_MARGINS_F16")) { float m0 = 0.f, m1 = 0.f; if (sscanf(env, "%f,%f", &m0, &m1) == 2 && m0 > 0.f && m1 > 0.f) { c->cert_margin_floor_f16[0] = m0; c->cert_margin_floor_f16[1] = m1; } }
    if (const char *env = getenv("NERF_CERTIFY_ZERO_TILES")) c->cert_zero_tiles = atoi(env) != 0;
    if (const char *env = getenv("NERF_CERTIFY_ZERO_FRAC")) { const double v = atof(env); if (v > 0.0 && v <= 1.0) c->cert_zero_frac = (float)v; }
    if (const char *env = getenv("NERF_CERTIFY_CUT_DEPTH")) { const double v = atof(env); if (v > 0.0) c->cert_depth_limit = (float)v; }
    if (const char *env = getenv("NERF_CERTIFY_AUDIT_MASK")) { const long v = atol(env); if (v >= 0 && ((v + 1) & v) == 0) c->cert_audit_mask = (unsigned)v; }
    if (const char *env = getenv("NERF_CERTIFY_AUDIT_MASK_NEAR")) { const long v = atol(env); if (v >= 0 && ((v + 1) & v) == 0) c->cert_audit_mask_near = (unsigned)v; }
    if (const char *env = getenv("NERF_CERTIFY_MARGINS")) {
        float m0 = 0.f, m1 = 0.f;
        if (sscanf(env, "%f,%f", &m0, &m1) == 2 && m0 > 0.f && m1 > 0.f) { c->cert_margin_floor[0] = m0; c->cert_margin_floor[1] = m1; c->cert_margin[0] = m0; c->cert_margin[1] = m1; }
    }
#endif
    env_size("NERF_GRADIENT_CHUNK", &c->gradient_chunk);
    if (const char *env = getenv("NERF_DEBUG_NORMALS")) c->debug_normals = atoi(env) > 0;
    if (const char *env = getenv("NERF_ZERO_STEP_SKIP")) c->zero_step_skip = atoi(env) != 0;
    if (const char *env = getenv("NERF_RAY_GROUPING")) c->ray_grouping = atoi(env) != 0;
    if (const char *env = getenv("NERF_WAVE_TILING")) c->wave_tiling = atoi(env) != 0;
    if (const char *env = getenv("NERF_DEPTH_ORDER")) c->depth_order = atoi(env) != 0;
    if (const char *env = getenv("NERF_TILE_ROTATION")) c->tile_rotation = atoi(env) != 0;
    if (const char *env = getenv("NERF_EMPTY_TILE_VOTE")) c->empty_tile_vote = atoi(env) != 0;
    if (const char *env = getenv("NERF_DEBUG_EMPTY_TILES")) c->debug_empty_tiles = atoi(env) > 0;
    if (const char *env = getenv("NERF_COARSE_CUT")) c->coarse_cut = atoi(env) <= 0 ? 0 : atoi(env) >= 2 ? 2 : 1;
    if (const char *env = getenv("NERF_DEBUG_COARSE_CUT")) c->debug_coarse_cut = atoi(env) > 0;
    if (const char *env = getenv("NERF_FINE_CUT")) c->fine_cut = atoi(env) <= 0 ? 0 : atoi(env) >= 2 ? 2 : 1;
    if (const char *env = getenv("NERF_DEBUG_FINE_CUT")) c->debug_fine_cut = atoi(env) > 0;
    if (const char *env = getenv("NERF_DEBUG_ZSKIP")) {
        if (atoi(env) > 0) {
            (void)c->buf[BUF_ZSKIP].ensure(c, 2 * sizeof(unsigned long long));
            c->empty_tile_vote = false; // the k-step counters describe the dense colour head: a voted-away head would take its k-steps out of both
            c->coarse_cut = 0;          // ... and every sample of the sampling launch
            c->fine_cut = 0;            // ... and of the fine launch
        }
    }
    if (const char *env = getenv("NERF_DEBUG_CLOCK")) {
        if (atoi(env) > 0) (void)c->buf[BUF_CLOCK].ensure(c, (size_t)c->n_cus * 2 * sizeof(unsigned long long));
        c->clock_coarse = atoi(env) == 2; // 2: the sampling (coarse) launch leaves its clocks instead of the fine one
    }
    (void)c->buf[BUF_SKIP].ensure(c, sizeof(unsigned long long)); // a counter that could not be allocated stays NULL: its statistic reads 0
    (void)c->buf[BUF_NONFINITE].ensure(c, sizeof(unsigned int));
    if (c->coarse_cut || c->fine_cut) (void)c->buf[BUF_CUT].ensure(c, 2 * sizeof(unsigned long long)); // without its counters a context renders without the cut
    // kernel attributes (dynamic LDS sizes) are per device, not per context: set them once per device and process
    static std::mutex init_mu;
    static std::set<int> init_done;
    hipError_t e1 = hipSuccess, e2 = hipSuccess;
    {
        std::lock_guard<std::mutex> lk(init_mu);
        if (!init_done.count(device_id)) {
            e1 = init_mlp_kernels();
            e2 = e1 == hipSuccess ? sampling_init() : e1;
            if (e2 == hipSuccess) init_done.insert(device_id);
        }
    }
    hipError_t e3 = e2 == hipSuccess ? hipStreamCreate(&c->stream) : e2;
    if (e3 != hipSuccess) {
        const std::string m = std::string("context initialisation failed: ") + hipGetErrorString(e3);
        nerf_destroy(c); // frees whatever was allocated so far (counters, clock buffer, stream)
        return fail(nullptr, NERF_ERR_HIP, m);
    }
    *out = c;
    return NERF_OK;
} NERF_CATCH(nullptr)

void nerf_destroy(nerf_ctx *c) {
    if (!c) return;
    DeviceGuard dg(c->device);
    (void)hipDeviceSynchronize();
    for (DevNet &n : c->net) for (DevBuf &b : n.buf) if (b.p) (void)hipFree(b.p);
    for (DevBuf &b : c->buf) if (b.p) (void)hipFree(b.p);
    recycle_render(c);
    recycle_dominant(c, 0);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int nerf_device_info(const nerf_ctx *c, int *n_cus, char *arch_name, size_t len) {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_cus) *n_cus = c->n_cus;
    if (arch_name && len) snprintf(arch_name, len, "%s", c->arch.c_str());
    return NERF_OK;
}

int nerf_band_rows(int window_rows, int band_index, int band_count, int band_stripe_rows) {
    if (window_rows < 0 || band_count < 0 || band_stripe_rows < 0 || (band_count > 1 && (band_index < 0 || band_index >= band_count)))
        return fail(nullptr, NERF_ERR_INVALID, "nerf_band_rows: bad argument");
    return band_rows(window_rows, band_index, band_count, band_stripe_rows);
}

int nerf_kernel_time_query(nerf_ctx *c, double *ms, uint64_t *points, uint32_t *n_launches, int reset) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    DeviceGuard dg(c->device);
    double tot = 0.0; uint64_t pts = 0; uint32_t nl = 0;
    for (const auto &p : c->dominant) {
        HIP_TRY(c, hipEventSynchronize(p.b));
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, p.a, p.b));
        tot += t; pts += p.points; ++nl;
    }
    if (ms) *ms = tot;
    if (points) *points = pts;
    if (n_launches) *n_launches = nl;
    if (reset) {
        // last_render may still list these pairs; it never recycles them, and they are not read again
        c->last_render.erase(std::remove_if(c->last_render.begin(), c->last_render.end(), [](const EvPair &p) { return p.dominant; }), c->last_render.end());
        recycle_dominant(c, 0);
    }
    return NERF_OK;
} NERF_CATCH(c)

int nerf_debug_shader_clock_mhz(nerf_ctx *c, double *mhz) try {
    if (!c || !mhz) return fail(c, NERF_ERR_INVALID, "NULL argument");
    if (!c->buf[BUF_CLOCK].p || !c->clock_valid) return fail(c, NERF_ERR_STATE, "set NERF_DEBUG_CLOCK=1 before nerf_create and render a frame first");
    DeviceGuard dg(c->device);
    std::vector<unsigned long long> h((size_t)c->n_cus * 2);
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(h.data(), c->buf[BUF_CLOCK].p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> f;
    for (int i = 0; i < c->n_cus; ++i) if (h[2 * i + 1] > 0) f.push_back(100.0 * (double)h[2 * i] / (double)h[2 * i + 1]);
    if (f.empty()) return fail(c, NERF_ERR_STATE, "no clock samples");
    std::sort(f.begin(), f.end());
    *mhz = f[f.size() / 2];
    return NERF_OK;
} NERF_CATCH(c)

int nerf_debug_workgroup_clocks(nerf_ctx *c, uint64_t *out, size_t n_workgroups) try {
    if (!c || !out) return fail(c, NERF_ERR_INVALID, "NULL argument");
    if (!c->buf[BUF_CLOCK].p || !c->clock_valid) return fail(c, NERF_ERR_STATE, "set NERF_DEBUG_CLOCK=1 (or 2) before nerf_create and render a frame first");
    if (n_workgroups > (size_t)c->n_cus) return fail(c, NERF_ERR_INVALID, "more workgroups than the context launches");
    DeviceGuard dg(c->device);
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(out, c->buf[BUF_CLOCK].p, n_workgroups * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return NERF_OK;
} NERF_CATCH(c)

} // extern "C"
