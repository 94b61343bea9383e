// nerf_api.cpp -- context, device memory, render scheduler and the extern "C" boundary (include/nerf_mi355x.h).
//
// Host counterpart of render_image / render_block (reference src/lib.rs:353-565): where the reference cuts the
// frame in 8x8 blocks for rayon workers, this scheduler cuts it in "passes" of whole ray rows (<= max_rays_per_pass
// rays, all resident in HBM) and runs per pass
//     ray dirs -> stratified t -> coarse MLP (sigma) -> resample/sort -> fine MLP -> composite
// as six launches on one stream with no host round trip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "components_kernels.h"
#include "host_util.h"
#include "isosurface_kernels.h"
#include "mlp_kernel.h"
#include "mlp_layout.h"
#include "normal_kernels.h"
#include "ray_batch_kernels.h"
#include "sampling_kernels.h"

using namespace nerfhost;

#include "nerf_internal.h"

using namespace nerfint;

namespace nerfint {

int fail(nerf_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return nerfhost::fail_noctx(code, msg); // also recorded for nerf_last_error(NULL) of this thread
}

} // namespace nerfint

namespace {

hipEvent_t get_event(nerf_ctx *c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Event pairs of kind 1 (dominant MLP kernel) are owned by ctx->dominant once a render has finished; every other
// pair is owned by ctx->last_render.
void recycle_render(nerf_ctx *c) {
    for (auto &p : c->last_render) if (p.kind != 1) { c->ev_pool.push_back(p.a); c->ev_pool.push_back(p.b); }
    c->last_render.clear();
}

void recycle_dominant(nerf_ctx *c, size_t keep) {
    while (c->dominant.size() > keep) {
        c->ev_pool.push_back(c->dominant.front().a); c->ev_pool.push_back(c->dominant.front().b);
        c->dominant.erase(c->dominant.begin());
    }
}

} // namespace

int nerfint::ensure_bytes(nerf_ctx *c, void **p, size_t *cur, size_t need) {
    if (*cur >= need) return NERF_OK;
    if (*p) { HIP_TRY(c, hipDeviceSynchronize()); HIP_TRY(c, hipFree(*p)); *p = nullptr; *cur = 0; }
    HIP_TRY(c, hipMalloc(p, need));
    *cur = need;
    return NERF_OK;
}

namespace {

// The coarse network's colours exist only in a coarse_only render (the reference discards them otherwise, src/lib.rs:404):
// their buffer (rays x nc x 3 floats, 492 MB for an 800x800 pass) is allocated on first such use only.
int ensure_workspace(nerf_ctx *c, size_t rays, size_t nc, size_t m, bool need_rgbc) {
    if (rays <= c->ws_rays && nc <= c->ws_nc && m <= c->ws_m && (!need_rgbc || c->d_rgbc)) return NERF_OK;
    rays = std::max(rays, c->ws_rays); nc = std::max(nc, c->ws_nc); m = std::max(m, c->ws_m);
    need_rgbc = need_rgbc || c->d_rgbc != nullptr;
    HIP_TRY(c, hipDeviceSynchronize());
    float **ptrs[] = {&c->d_dirs, &c->d_tc, &c->d_sc, &c->d_rgbc, &c->d_tf, &c->d_sf, &c->d_rgbf};
    for (auto p : ptrs) if (*p) { HIP_TRY(c, hipFree(*p)); *p = nullptr; }
    c->ws_rays = c->ws_nc = c->ws_m = 0;
    HIP_TRY(c, hipMalloc((void **)&c->d_dirs, rays * 3 * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_tc, rays * nc * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_sc, rays * nc * sizeof(float)));
    if (need_rgbc) HIP_TRY(c, hipMalloc((void **)&c->d_rgbc, rays * nc * 3 * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_tf, rays * m * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_sf, rays * m * sizeof(float)));
    HIP_TRY(c, hipMalloc((void **)&c->d_rgbf, rays * m * 3 * sizeof(float)));
    c->ws_rays = rays; c->ws_nc = nc; c->ws_m = m;
    return NERF_OK;
}

int upload_packed(nerf_ctx *c, int which, const std::vector<float> &ws, const std::vector<float> &sm);

// The bf16 kernel: mlp_kernel_bf16v2.hip (32x32x16).  A variant build with -DNERF_BF16_V3=1 (make variant; round-3 experiment, see
// DESIGN 4.3) links mlp_kernel_bf16v3.hip (16x16x32) instead: same arithmetic, same results, measured 6 % slower on the full kernel.
#ifndef NERF_BF16_V3
#define NERF_BF16_V3 0
#endif
static constexpr bool g_bf16_v2 = !NERF_BF16_V3;

// weight stream + launcher of the selected arithmetic
static bool valid_dtype(int d) { return d == NERF_MLP_F32 || d == NERF_MLP_BF16 || d == NERF_MLP_BF16X3 || d == NERF_MLP_F16X2; }
static bool split_dtype(int d) { return d == NERF_MLP_BF16X3 || d == NERF_MLP_F16X2; } // f32-accurate operand-splitting arithmetics
static const float *stream_of(const DevNet &n, int dtype) {
    if (dtype == NERF_MLP_BF16X3) return (const float *)n.wstream_x3;
    if (dtype == NERF_MLP_F16X2) return (const float *)n.wstream_x2;
    if (dtype == NERF_MLP_F32) return n.wstream;
    return g_bf16_v2 ? (const float *)n.wstream_bf16v2 : (const float *)n.wstream_bf16v3;
}
// the small block that goes with stream_of: the f32 kernels read the folded image, every other arithmetic the packed one
static const float *small_of(const DevNet &n, int dtype) { return dtype == NERF_MLP_F32 ? n.small_f32 : n.small; }
// zero-step skipping of the f32 kernels (MlpArgs / SeqArgs; the other arithmetics ignore the two fields): per network, decided at load
// ... and the context's ray grouping (MlpArgs.ray_grouping: the ray-mode launcher of the f32 kernels reads it, nothing else does)
static void grouping_of(const nerf_ctx *c, MlpArgs &a) { a.ray_grouping = c->ray_grouping ? 1 : 0; }
static void grouping_of(const nerf_ctx *, SeqArgs &) {}
template <class Args>
static void zskip_of(const nerf_ctx *c, const DevNet &n, Args &a) { a.zero_skip = n.zero_skip ? 1 : 0; a.zskip_stats = c->d_zskip; grouping_of(c, a); }
// NERF_V2_F16_FULL (experiment, variant builds): NERF_MLP_BF16 renders run the f16 twin of the bf16 kernel (fused ray-mode launches only)
static hipError_t launch_mlp(const nerf_ctx *c, int dtype, const MlpArgs &a, bool full, hipStream_t st) {
#ifdef NERF_V2_F16_FULL
    if (dtype == NERF_MLP_BF16 && a.mode == MLP_MODE_RAYS && !a.raw_pre) {
        MlpArgs b = a;
        for (const DevNet &n : c->net) if ((const void *)n.wstream_bf16v2 == (const void *)a.wstream && n.wstream_f16v2) b.wstream = (const float *)n.wstream_f16v2;
        return full ? nerf_mlp_f16v2_full_launch(b, c->n_cus, st) : nerf_mlp_f16v2_launch(b, c->n_cus, st);
    }
#endif
    if (dtype == NERF_MLP_F32) return nerf_mlp_launch(a, full, c->n_cus, st);
    if (dtype == NERF_MLP_BF16X3) return nerf_mlp_bf16x3_launch(a, full, c->n_cus, st);
    if (dtype == NERF_MLP_F16X2) return nerf_mlp_f16x2_launch(a, full, c->n_cus, st);
#if NERF_BF16_V3
    return nerf_mlp_bf16v3_launch(a, full, c->n_cus, st);
#else
    return nerf_mlp_bf16v2_launch(a, full, c->n_cus, st);
#endif
}

// v1 stream -> v2 stream: the 1-KiB pieces are identical (lane l, element j = W[row(tile, 8 ks + j, l >> 5)][32 nt + (l & 31)]);
// v1 orders a layer's pieces (k-step, nt), v2 orders them (nt, k-step) and pads viewdirs' 72 pieces to 80.
static void bf16_v2_from_v1(const std::vector<uint16_t> &v1, std::vector<uint16_t> &v2) {
    using namespace nerfmlp;
    v2.clear();
    v2.reserve((size_t)kChunksFullBf16V2 * kChunkBytesBf16V2 / 2);
    size_t base = 0; // uint16 elements
    auto layer = [&](int KS, int NT) {
        for (int nt = 0; nt < NT; ++nt)
            for (int ks = 0; ks < KS; ++ks) {
                const uint16_t *src = &v1[base + ((size_t)ks * NT + nt) * 512];
                v2.insert(v2.end(), src, src + 512);
            }
        base += (size_t)KS * NT * 512;
    };
    layer(4, 8);
    for (int i = 0; i < 4; ++i) layer(16, 8);
    layer(20, 8);
    for (int i = 0; i < 3; ++i) layer(16, 8);
    layer(18, 4);
    v2.resize((size_t)kChunksFullBf16V2 * kChunkBytesBf16V2 / 2, (uint16_t)0);
}

// v1 order (f32 values) -> the stream of mlp_kernel_bf16v3.hip (v_mfma_f32_16x16x32_bf16): per layer, per output tile nt, per k-step ks
// (K = 32), per 16-feature half fh one 1-KiB piece: lane l = (i = l & 15, g = l >> 4), element e = W[row(ks, g, e)][32 nt + 16 fh + i].
// Hidden k-steps: k-slot (g, e) = feature 4 g + e (e < 4) or 16 + 4 g + e - 4 of input tile ks (the C/D layout of two 16x16 output
// halves packed pairwise); encoding k-steps: slot 32 ks + 8 g + e = the reference's feature index (src/network.rs:263-330).
static void bf16_v3_from_v1(const std::vector<float> &v1f, std::vector<uint16_t> &v3) {
    using namespace nerfmlp;
    v3.clear();
    v3.reserve((size_t)kChunksFullBf16V2 * kChunkBytesBf16V2 / 2);
    int pos_inv[64][3], dir_inv[32][3]; // reference feature -> (input tile, register, lane-half) of the 32x32 layouts
    for (auto &x : pos_inv) x[0] = -1;
    for (auto &x : dir_inv) x[0] = -1;
    for (int tt = 0; tt < 2; ++tt)
        for (int r = 0; r < 16; ++r)
            for (int h = 0; h < 2; ++h) {
                const int f = posSlotFeature(16 * tt + r, h);
                if (f >= 0) { pos_inv[f][0] = tt; pos_inv[f][1] = r; pos_inv[f][2] = h; }
            }
    for (int r = 0; r < 16; ++r)
        for (int h = 0; h < 2; ++h) {
            const int f = dirSlotFeature(r, h);
            if (f >= 0) { dir_inv[f][0] = 0; dir_inv[f][1] = r; dir_inv[f][2] = h; }
        }
    size_t base = 0; // v1 pieces
    // kind of k-step ks: 0 = activation tile `tile`, 1 = position-encoding slots 32 * tile .., 2 = direction-encoding slots
    auto layer = [&](int n_tiles_v1, int NT, int KS, auto kind_of) {
        for (int nt = 0; nt < NT; ++nt)
            for (int ks = 0; ks < KS; ++ks)
                for (int fh = 0; fh < 2; ++fh)
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 8; ++e) {
                            const int i = l & 15, g = l >> 4;
                            int kind, tile;
                            kind_of(ks, kind, tile);
                            int tt = -1, r = 0, h = 0;
                            if (kind == 0) {
                                const int f = e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4);
                                tt = tile; h = (f >> 2) & 1; r = (f & 3) + 4 * (f >> 3);
                            } else if (kind == 1) {
                                const int s = 32 * tile + 8 * g + e;
                                if (s < 63 && pos_inv[s][0] >= 0) { tt = pos_inv[s][0]; r = pos_inv[s][1]; h = pos_inv[s][2]; }
                            } else {
                                const int s = 8 * g + e;
                                if (s < 27 && dir_inv[s][0] >= 0) { tt = n_tiles_v1 - 1; r = dir_inv[s][1]; h = dir_inv[s][2]; }
                            }
                            float v = 0.0f;
                            if (tt >= 0) {
                                const size_t piece = base + ((size_t)(tt * 2 + (r >> 3)) * NT + nt);
                                v = v1f[(piece * 64 + (size_t)(16 * fh + i + 32 * h)) * 8 + (r & 7)];
                            }
                            v3.push_back(f32_to_bf16_rne(v));
                        }
        base += (size_t)n_tiles_v1 * 2 * NT;
    };
    layer(2, 8, 2, [](int ks, int &kind, int &tile) { kind = 1; tile = ks; });
    for (int i = 0; i < 4; ++i) layer(8, 8, 8, [](int ks, int &kind, int &tile) { kind = 0; tile = ks; });
    layer(10, 8, 10, [](int ks, int &kind, int &tile) { if (ks < 2) { kind = 1; tile = ks; } else { kind = 0; tile = ks; } });
    for (int i = 0; i < 3; ++i) layer(8, 8, 8, [](int ks, int &kind, int &tile) { kind = 0; tile = ks; });
    layer(9, 4, 9, [](int ks, int &kind, int &tile) { if (ks < 8) { kind = 0; tile = ks; } else { kind = 2; tile = 0; } });
    v3.resize((size_t)kChunksFullBf16V2 * kChunkBytesBf16V2 / 2, (uint16_t)0);
}

// All bf16-family streams come from one f32 array in the first bf16 design's piece order (host_util.h).
int upload_bf16_family(nerf_ctx *c, int which, const std::vector<float> &v1f) {
    if (v1f.size() != (size_t)nerfmlp::kPiecesV1 * 512) return fail(c, NERF_ERR_SHAPE, "internal: bf16 piece array has the wrong size");
    DevNet &d = c->net[which];
    std::vector<uint16_t> wb, v2, x3;
    bf16_stream_from_v1order(v1f, wb);
    bf16_v2_from_v1(wb, v2);
    x3_stream_from_v1order(v1f, x3);
    if (x3.size() != (size_t)nerfmlp::kChunksFullX3 * nerfmlp::kChunkBytesX3 / 2) return fail(c, NERF_ERR_SHAPE, "internal: bf16x3 stream size");
    if (!d.wstream_bf16v2) HIP_TRY(c, hipMalloc((void **)&d.wstream_bf16v2, v2.size() * sizeof(uint16_t)));
    HIP_TRY(c, hipMemcpy(d.wstream_bf16v2, v2.data(), v2.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    if (!g_bf16_v2) {
        std::vector<uint16_t> v3;
        bf16_v3_from_v1(v1f, v3);
        if (v3.size() != v2.size()) return fail(c, NERF_ERR_SHAPE, "internal: bf16 v3 stream size");
        if (!d.wstream_bf16v3) HIP_TRY(c, hipMalloc((void **)&d.wstream_bf16v3, v3.size() * sizeof(uint16_t)));
        HIP_TRY(c, hipMemcpy(d.wstream_bf16v3, v3.data(), v3.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    if (!d.wstream_x3) HIP_TRY(c, hipMalloc((void **)&d.wstream_x3, x3.size() * sizeof(uint16_t)));
    HIP_TRY(c, hipMemcpy(d.wstream_x3, x3.data(), x3.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    {   // the f16 twin of the bf16 v2 stream (certify_zero's pre-filter): the same pieces in the same order, f16-rounded
        std::vector<uint16_t> hb, h2;
        const bool fits = f16_stream_from_v1order(v1f, hb);
        if (fits) {
            bf16_v2_from_v1(hb, h2); // a permutation of 16-bit elements: the element type does not matter
            if (h2.size() != v2.size()) return fail(c, NERF_ERR_SHAPE, "internal: f16 v2 stream size");
            if (!d.wstream_f16v2) HIP_TRY(c, hipMalloc((void **)&d.wstream_f16v2, h2.size() * sizeof(uint16_t)));
            HIP_TRY(c, hipMemcpy(d.wstream_f16v2, h2.data(), h2.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        } else if (d.wstream_f16v2) {
            HIP_TRY(c, hipFree(d.wstream_f16v2));
            d.wstream_f16v2 = nullptr;
        }
        // certify_zero calibrates itself per network: margins start at the floors of the pre-filter this network gets
        c->cert_prefilter_f16[which] = g_bf16_v2 && c->cert_allow_f16 && d.wstream_f16v2 != nullptr;
        c->cert_margin[which] = c->cert_prefilter_f16[which] ? c->cert_margin_floor_f16[which] : c->cert_margin_floor[which];
    }
    std::vector<uint16_t> x2;
    if (x2_stream_from_v1order(v1f, x2)) { // every weight inside the f16 range (the lego networks: |w| <= 8.3)
        if (x2.size() != (size_t)nerfmlp::kChunksFullF16X2 * nerfmlp::kChunkBytesF16X2 / 2) return fail(c, NERF_ERR_SHAPE, "internal: f16x2 stream size");
        if (!d.wstream_x2) HIP_TRY(c, hipMalloc((void **)&d.wstream_x2, x2.size() * sizeof(uint16_t)));
        HIP_TRY(c, hipMemcpy(d.wstream_x2, x2.data(), x2.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    } else if (d.wstream_x2) { // a reload with out-of-range weights: NERF_MLP_F16X2 becomes unavailable for this network
        HIP_TRY(c, hipFree(d.wstream_x2));
        d.wstream_x2 = nullptr;
    }
    return NERF_OK;
}

int upload_net(nerf_ctx *c, int which, const HostNet &hn) {
    std::vector<float> ws, sm;
    pack_network(hn, ws, sm);
    int rc = upload_packed(c, which, ws, sm);
    if (rc) return rc;
    std::vector<float> v1f;
    pack_network_v1order_f32(hn, v1f);
    return upload_bf16_family(c, which, v1f);
}

// The bf16-family streams hold the same weights in another order; for networks that arrive as a packed f32 blob they are
// rebuilt from the f32 stream's pieces (piece (s, g): lane l, q -> W[row(s, l >> 5)][32 (4 g + q) + (l & 31)]).
int bf16_from_f32_stream(nerf_ctx *c, int which, const std::vector<float> &ws) {
    using namespace nerfmlp;
    std::vector<float> v1f;
    v1f.reserve((size_t)kPiecesV1 * 512);
    size_t layer_base = 0; // floats
    auto layer = [&](int n_tiles, int NT) {
        for (int tt = 0; tt < n_tiles; ++tt)
            for (int ks = 0; ks < 2; ++ks)
                for (int nt = 0; nt < NT; ++nt)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int st = 16 * tt + 8 * ks + j; // f32 k-step that holds register 8 ks + j of tile tt
                            const size_t piece = layer_base + ((size_t)st * (NT / 4) + nt / 4) * 256;
                            v1f.push_back(ws[piece + (size_t)l * 4 + (nt & 3)]);
                        }
        layer_base += (size_t)n_tiles * 16 * NT * 64;
    };
    layer(2, 8);
    for (int i = 0; i < 4; ++i) layer(8, 8);
    layer(10, 8);
    for (int i = 0; i < 3; ++i) layer(8, 8);
    layer(9, 4);
    return upload_bf16_family(c, which, v1f);
}

int upload_packed(nerf_ctx *c, int which, const std::vector<float> &ws, const std::vector<float> &sm) {
    if (ws.size() != (size_t)nerfmlp::kChunksFull * nerfmlp::kChunkFloats || sm.size() != (size_t)nerfmlp::kSmallFloats)
        return fail(c, NERF_ERR_SHAPE, "packed network image has the wrong size for this library build");
    // the f32 kernels run the bottleneck folded into viewdirs (once per loaded network); the 16-bit arithmetics keep the packed
    // image's small block (their streams come from upload_bf16_family)
    std::vector<float> fws, fsm;
    if (!fold_network(ws, sm, fws, fsm)) return fail(c, NERF_ERR_SHAPE, "internal: folded network image has the wrong size");
    DevNet &d = c->net[which];
    if (!d.wstream) HIP_TRY(c, hipMalloc((void **)&d.wstream, fws.size() * sizeof(float)));
    if (!d.small) HIP_TRY(c, hipMalloc((void **)&d.small, sm.size() * sizeof(float)));
    if (!d.small_f32) HIP_TRY(c, hipMalloc((void **)&d.small_f32, fsm.size() * sizeof(float)));
    HIP_TRY(c, hipMemcpy(d.wstream, fws.data(), fws.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.small, sm.data(), sm.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.small_f32, fsm.data(), fsm.size() * sizeof(float), hipMemcpyHostToDevice));
    d.loaded = true;
    d.zero_skip = c->zero_step_skip && zero_skip_safe(fws, fsm); // exact only while every parameter is finite (mlp_f32_core.hip.h tile_steps)
    c->cert_margin[which] = c->cert_margin_floor[which]; // certify_zero calibrates itself per network (upload_bf16_family, which follows, decides the pre-filter)
    return NERF_OK;
}

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

// Record kernel(s) between two events of the given kind.  If done() is never reached (a launch failed and the caller
// returned early) the destructor hands the events back to the pool.
struct Timed {
    nerf_ctx *c; hipStream_t st; EvPair p; bool on;
    Timed(nerf_ctx *c_, hipStream_t st_, int kind, uint64_t points, bool enable) : c(c_), st(st_), on(enable) {
        p.kind = kind; p.points = points; p.a = get_event(c); p.b = get_event(c);
        if (!p.a || !p.b) on = false;
        if (on) (void)hipEventRecord(p.a, st);
    }
    Timed(const Timed &) = delete;
    Timed &operator=(const Timed &) = delete;
    void done(std::vector<EvPair> &dst) {
        if (on) { (void)hipEventRecord(p.b, st); dst.push_back(p); p.a = p.b = nullptr; }
    }
    ~Timed() {
        if (p.a) c->ev_pool.push_back(p.a);
        if (p.b) c->ev_pool.push_back(p.b);
    }
};

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

int render_once(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, float *d_out, float *d_depth, float *d_opacity, hipStream_t st,
                nerf_stats *stats, CertOutcome *cert, const float *background) {
    int rc;
    if ((rc = check_camera(c, cam))) return rc;
    if (!o) return fail(c, NERF_ERR_INVALID, "opts is NULL");
    if (!d_out) return fail(c, NERF_ERR_INVALID, "output pointer is NULL");
    if (o->n_coarse <= 0) return fail(c, NERF_ERR_INVALID, "coarse samples per ray must be greater than 0"); // src/lib.rs:483-486
    if (o->n_fine < 0) return fail(c, NERF_ERR_INVALID, "fine samples per ray must be >= 0");
    if (!valid_dtype(o->mlp_dtype)) return fail(c, NERF_ERR_INVALID, "mlp_dtype must be NERF_MLP_F32, NERF_MLP_BF16, NERF_MLP_BF16X3 or NERF_MLP_F16X2");
    const int dtype = o->mlp_dtype;
    // bf16x3 / f16x2: the sampling pass (coarse sigma -> CDF -> fine sample positions) stays on the exact-f32 MFMA kernel, so the fine
    // samples sit where the f32 path puts them bit for bit (a 1e-5 density difference can move a CDF entry across a fixed
    // uniform draw and relocate a sample -- a discontinuity, not an accuracy problem); only the colour-producing pass runs in
    // the three-way split arithmetic.
    // hybrid_sampling: the sampling pass itself runs in a split arithmetic (the render's own, or -- for an f32 render -- f16x2 where
    // the network fits the f16 range, else bf16x3) and only the ill-conditioned rays are redone in f32.
    const int dtype_coarse = o->hybrid_sampling ? (split_dtype(dtype) ? dtype : c->net[NERF_NET_COARSE].wstream_x2 ? NERF_MLP_F16X2 : NERF_MLP_BF16X3)
                                                : (split_dtype(dtype) && !o->coarse_only) ? NERF_MLP_F32 : dtype;
    if (o->skip_empty != 0 && o->skip_empty != 1) return fail(c, NERF_ERR_INVALID, "skip_empty must be 0 or 1");
    if (o->skip_dead != 0 && o->skip_dead != 1) return fail(c, NERF_ERR_INVALID, "skip_dead must be 0 or 1");
    const bool seq = o->skip_dead != 0;
    if (seq && dtype == NERF_MLP_BF16 && !g_bf16_v2) return fail(c, NERF_ERR_INVALID, "skip_dead with NERF_MLP_BF16 is not part of the NERF_BF16_V3 variant build");
    if (o->hybrid_sampling != 0 && o->hybrid_sampling != 1) return fail(c, NERF_ERR_INVALID, "hybrid_sampling must be 0 or 1");
    if (o->certify_zero != 0 && o->certify_zero != 1) return fail(c, NERF_ERR_INVALID, "certify_zero must be 0 or 1");
    if (o->certify_zero && (dtype == NERF_MLP_BF16 || seq || o->skip_empty || !g_bf16_v2))
        return fail(c, NERF_ERR_INVALID, "certify_zero needs mlp_dtype F32, BF16X3 or F16X2 and neither skip_empty nor skip_dead");
    if (o->hybrid_sampling && !(seq && !o->coarse_only && dtype != NERF_MLP_BF16)) // bf16 is its own arithmetic: there are no f32 sample positions to protect
        return fail(c, NERF_ERR_INVALID, "hybrid_sampling needs skip_dead = 1, mlp_dtype F32, BF16X3 or F16X2, and a hierarchical render");
    if (!c->net[NERF_NET_COARSE].loaded) return fail(c, NERF_ERR_STATE, "coarse network not loaded");
    if (!o->coarse_only && !c->net[NERF_NET_FINE].loaded) return fail(c, NERF_ERR_STATE, "fine network not loaded");
    if (dtype == NERF_MLP_F16X2 && (!c->net[o->coarse_only ? NERF_NET_COARSE : NERF_NET_FINE].wstream_x2 ||
                                    (o->hybrid_sampling && !c->net[NERF_NET_COARSE].wstream_x2)))
        return fail(c, NERF_ERR_STATE, "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range");
    const int s = o->ssaa > 1 ? o->ssaa : 1;
    int x0 = 0, y0 = 0, cw = cam->nx, ch = cam->ny;
    if (o->crop_w > 0 || o->crop_h > 0) { x0 = o->crop_x0; y0 = o->crop_y0; cw = o->crop_w; ch = o->crop_h; }
    if (cw <= 0 || ch <= 0 || x0 < 0 || y0 < 0 || x0 + cw > cam->nx || y0 + ch > cam->ny)
        return fail(c, NERF_ERR_INVALID, "crop window outside the frame");
    // one band of the window's rows (multi-GPU): contiguous bands are just a shorter window; striped bands keep the window and map
    // band-local rows to window rows in the ray generator (sampling_kernels.hip ray_row)
    int stripe = 0;
    if (o->band_count > 1) {
        if (o->band_index < 0 || o->band_index >= o->band_count || o->band_stripe_rows < 0) return fail(c, NERF_ERR_INVALID, "band_index / band_count / band_stripe_rows out of range");
        const int rows = band_rows(ch, o->band_index, o->band_count, o->band_stripe_rows);
        if (rows <= 0) return fail(c, NERF_ERR_INVALID, "this band has no rows (more bands than rows)");
        if (o->band_stripe_rows == 0) y0 += band_first_row(ch, o->band_index, o->band_count);
        else stripe = o->band_stripe_rows;
        ch = rows;
    } else if (o->band_count < 0) return fail(c, NERF_ERR_INVALID, "band_count must be >= 0");
    const int nc = o->n_coarse;
    // sample_importance returns nothing for count == 0 or < 3 coarse samples (src/lib.rs:295-297): the fine net
    // then runs on the coarse samples only
    const int nf = (o->coarse_only || o->n_fine == 0 || nc < 3) ? 0 : o->n_fine;
    const int M = nc + nf;
    const bool hybrid = o->hybrid_sampling != 0 && nf > 0; // without resampling there is nothing to protect
    if (composite_lds_bytes(M) > 160 * 1024 || (nf > 0 && resample_lds_bytes(nc, nf) > 160 * 1024))
        return fail(c, NERF_ERR_INVALID, "too many samples per ray for the sampling / compositing kernels (one ray per wave in LDS)");
    const int RW = cw * s, RH = ch * s, RX0 = x0 * s, RY0 = y0 * s;
    // a pass must keep rays * samples within int32 (kernel indices) as well as within the configured budget
    size_t pass_cap = std::min<size_t>(c->max_rays_per_pass, (size_t)0x3fffffff / (size_t)M);
    // skip_dead in a split arithmetic or in bf16 (two launches): the compacted trunk outputs are sized for the worst case (every sample
    // of a pass live; 1 KiB each as f32 tiles, 512 B as packed bf16).  The f32 kernel compacts in LDS and runs its colour passes in the
    // same launch: no buffer, no extra passes.
    const bool h8_export = seq && (split_dtype(dtype) || dtype == NERF_MLP_BF16);
    const size_t h8_sample_bytes = dtype == NERF_MLP_BF16 ? 512 : 1024;
    // Budget and allocation of that buffer are ONE critical section per process: contexts that share a device (nerf_render_image_multi's
    // worker threads) would otherwise each claim half of the same free memory and fail in hipMalloc.  A context keeps its buffer while
    // later renders fit; a render that needs less than a quarter of it gives it back (shrinks).
    static std::mutex h8_mu;
    std::unique_lock<std::mutex> h8_lock(h8_mu, std::defer_lock);
    if (h8_export) {
        h8_lock.lock();
        size_t budget = c->max_export_bytes, free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) // never more than half of what the device can still give (plus what we already hold)
            budget = std::min(budget, (free_b + c->h8_bytes) / 2);
        const size_t row_bytes = (size_t)RW * M * h8_sample_bytes;
        if (row_bytes > budget) {
            char msg[256];
            snprintf(msg, sizeof msg, "skip_dead in this arithmetic exports %zu B per sample: one ray row of this render (%d rays x %d samples) needs "
                     "%zu MiB, the budget is %zu MiB (NERF_MAX_EXPORT_BYTES, free device memory / 2); render a narrower crop or use NERF_MLP_F32",
                     h8_sample_bytes, RW, M, row_bytes >> 20, budget >> 20);
            return fail(c, NERF_ERR_INVALID, msg);
        }
        pass_cap = std::min<size_t>(pass_cap, budget / ((size_t)M * h8_sample_bytes));
    }
    if ((size_t)RW > pass_cap && (size_t)RW * M > (size_t)0x3fffffff) return fail(c, NERF_ERR_INVALID, "ray row too wide for one pass");
    const size_t rows_per_pass = std::max<size_t>(1, std::min<size_t>(RH, pass_cap / (size_t)RW));
    if ((rc = ensure_workspace(c, rows_per_pass * RW, nc, M, o->coarse_only != 0))) return rc;
    float *ray_out = d_out, *ray_depth = d_depth, *ray_opacity = d_opacity;
    if (s > 1) {
        if ((rc = ensure_bytes(c, (void **)&c->d_rayfb, &c->rayfb_floats, (size_t)RW * RH * 3 * sizeof(float)))) return rc;
        ray_out = c->d_rayfb;
        if (d_depth || d_opacity) { // ray-level maps, one plane each, box-filtered like the colour below
            if ((rc = ensure_bytes(c, (void **)&c->d_rayaux, &c->rayaux_bytes, (size_t)RW * RH * 2 * sizeof(float)))) return rc;
            ray_depth = d_depth ? c->d_rayaux : nullptr;
            ray_opacity = d_opacity ? c->d_rayaux + (size_t)RW * RH : nullptr;
        }
    }
    const uint32_t n_passes_total = (uint32_t)((RH + rows_per_pass - 1) / rows_per_pass);
    if (seq) { // per MLP launch: {u32 ray queue head, u32 live-sample count, u64 evaluated samples}
        const size_t slots = (size_t)n_passes_total * 3; // per pass: coarse, fine, hybrid f32 redo of the coarse pass
        if (slots > c->seq_slots) {
            size_t bytes = c->seq_slots * 16;
            if ((rc = ensure_bytes(c, (void **)&c->d_seq, &bytes, slots * 16))) return rc;
            c->seq_slots = slots;
        }
        HIP_TRY(c, hipMemsetAsync(c->d_seq, 0, slots * 16, st));
        const size_t pass_samples = rows_per_pass * RW * (size_t)M;
        if (h8_export) {
            const size_t need = dtype == NERF_MLP_BF16 ? nerf_seq_h8_bytes_bf16(pass_samples) : nerf_seq_h8_bytes(pass_samples);
            if (c->d_h8 && need < c->h8_bytes / 4) { // a much smaller render: give the big buffer back
                HIP_TRY(c, hipDeviceSynchronize());
                HIP_TRY(c, hipFree(c->d_h8));
                c->d_h8 = nullptr; c->h8_bytes = 0;
            }
            if ((rc = ensure_bytes(c, (void **)&c->d_h8, &c->h8_bytes, need))) return rc;
            if ((rc = ensure_bytes(c, (void **)&c->d_slot_point, &c->slot_point_bytes, (pass_samples + 256) * sizeof(unsigned int)))) return rc;
            h8_lock.unlock();
        }
        if (hybrid && (rc = ensure_bytes(c, (void **)&c->d_flag_list, &c->flag_list_bytes, rows_per_pass * RW * sizeof(unsigned int)))) return rc;
    }
    // Zero certification (nerf_render_opts.certify_zero; DESIGN 4.9, protocol: sampling_kernels.hip k_cert_*): a 16-bit pass (f16 or bf16 operands, cert_prefilter_f16) over all samples
    // finds (Z) the samples whose density pre-activation is so far below 0 (margin per network, c->cert_margin: audited every frame and
    // widened by render_device when the audit's headroom shrinks) that the exact network's density is certainly 0 there too, and predicts
    // (C) where each ray's transmittance falls below the reference's 1e-4 cut; the exact kernel evaluates only the remaining samples in
    // front of the predicted cut (a device-side list), the exact transmittance confirms the cut (or a second launch evaluates the rest).
    // A certified sample has sigma = 0 => weight 0, a sample behind the cut has weight 0 whatever its density: the frame is the plain
    // frame, bit for bit, as long as no certificate is wrong.
    const bool certify = o->certify_zero != 0;
    // per (pass, network): {list 1 length, list 2 length, audited, violations, headroom code, max-error bits, fallback rays, audit-record count,
    //                       pre-filter ray queue head, list 1 back-part length, u64 samples the pre-filter evaluated, ...}
    constexpr int kCertSlots = 16;
    size_t aux_cap = 0;
    size_t cert_cap = 0;
    if (certify) {
        if (cert_plan_lds_bytes(M, nullptr) > 159 * 1024) return fail(c, NERF_ERR_INVALID, "certify_zero: too many samples per ray");
        const size_t n_pass = ((size_t)RH + rows_per_pass - 1) / rows_per_pass;
        const size_t pass_samples = rows_per_pass * RW * (size_t)M;
        // the list is sized from what earlier frames needed (c->cert_list_frac of the samples, +25 %): if a pass wants more, the entries
        // beyond the capacity are counted, not stored, and render_device renders the frame again with a list that fits
        // (up to 64 MiB the list simply holds every sample: small renders -- a central crop lists 70 % of its samples -- never take that path)
        cert_cap = pass_samples <= ((size_t)16 << 20) ? pass_samples : std::min<size_t>(pass_samples, (size_t)((double)pass_samples * c->cert_list_frac) + 4096);
        if ((rc = ensure_bytes(c, (void **)&c->d_point_list, &c->point_list_bytes, cert_cap * sizeof(unsigned int)))) return rc;
        cert_cap = std::min<size_t>(pass_samples, c->point_list_bytes / sizeof(unsigned int)); // an earlier, larger allocation is kept
        if ((rc = ensure_bytes(c, (void **)&c->d_jstar, &c->jstar_bytes, rows_per_pass * RW * sizeof(int)))) return rc;
        aux_cap = 2 * (pass_samples / ((size_t)std::min(c->cert_audit_mask, c->cert_audit_mask_near) + 1)) + 4096; // more than the audit can select: a certificate that does not fit is not audited
        if ((rc = ensure_bytes(c, (void **)&c->d_cert_aux, &c->cert_aux_bytes, aux_cap * 2 * sizeof(unsigned int)))) return rc;
        if ((rc = ensure_bytes(c, (void **)&c->d_cert, &c->cert_bytes, kCertSlots * 2 * n_pass * sizeof(unsigned int)))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_cert, 0, kCertSlots * 2 * n_pass * sizeof(unsigned int), st));
        if (cert) { cert->list_capacity = cert_cap; cert->pass_samples = pass_samples; }
    }
    recycle_render(c);
    recycle_dominant(c, 4096); // bound the backlog if the caller never queries
    // If this render returns early (a launch failed), its dominant-kernel event pairs never reach c->dominant: hand them back
    // to last_render's ownership so that the next recycle_render returns them to the pool.
    struct RenderScope {
        nerf_ctx *c; bool ok = false;
        ~RenderScope() { if (!ok) for (auto &p : c->last_render) if (p.kind == 1) p.kind = 2; }
    } scope{c};
    if ((o->skip_empty || certify) && c->d_skip) HIP_TRY(c, hipMemsetAsync(c->d_skip, 0, sizeof(unsigned long long), st));
    const bool watch_range = c->d_nonfinite && (split_dtype(dtype) || split_dtype(dtype_coarse));
    if (watch_range) HIP_TRY(c, hipMemsetAsync(c->d_nonfinite, 0, sizeof(unsigned int), st));
    const bool timing = true;
    RayGenArgs g = make_raygen(*cam, s);
    if (stripe > 0) { g.stripe = stripe * s; g.stripe_n = o->band_count; g.stripe_i = o->band_index; g.stripe_y0 = RY0; }
    const DevNet &NC = c->net[NERF_NET_COARSE], &NF = c->net[NERF_NET_FINE];
    uint32_t passes = 0;
    for (int row = 0; row < RH; row += (int)rows_per_pass, ++passes) {
        const int rows = std::min<int>((int)rows_per_pass, RH - row);
        const int n_rays = rows * RW;
        g.n_rays = n_rays; g.rx0 = RX0; g.ry0 = (stripe > 0 ? 0 : RY0) + row; g.rw = RW;
        {
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_ray_dirs(g, c->d_dirs, st));
            HIP_TRY(c, launch_stratified(g, nc, cam->near_, cam->far_, o->seed, c->d_tc, st));
            t.done(c->last_render);
        }
        // skip_dead: one network over the rays of this pass as ray-sequential trunk [+ colour head on the live samples]
        auto seq_pass = [&](const DevNet &net, int dt, int spr, const float *t_in, float *sigma_out, float *rgb_out, int slot, int kind_trunk) -> int {
            unsigned int *ctr = c->d_seq + 4 * (size_t)slot;
            HIP_TRY(c, hipMemsetAsync(sigma_out, 0, (size_t)n_rays * spr * sizeof(float), st)); // samples behind the cut stay 0
            if (rgb_out) HIP_TRY(c, hipMemsetAsync(rgb_out, 0, (size_t)n_rays * spr * 3 * sizeof(float), st)); // weight-0 samples: 0 * 0
            SeqArgs q{};
            q.wstream = stream_of(net, dt); q.small_params = small_of(net, dt); zskip_of(c, net, q); q.n_rays = n_rays; q.samples_per_ray = spr;
            q.ray_dirs = c->d_dirs; q.t = t_in; q.far_ = cam->far_;
            q.origin[0] = cam->pos[0]; q.origin[1] = cam->pos[1]; q.origin[2] = cam->pos[2];
            q.sigma_out = sigma_out; q.ray_counter = ctr; q.live_count = ctr + 1; q.h8 = c->d_h8; q.slot_point = c->d_slot_point;
            q.rgb_out = rgb_out; // f32: colour passes inside the trunk launch
            q.stats = (unsigned long long *)(ctr + 2);
            q.nonfinite = split_dtype(dt) ? c->d_nonfinite : nullptr;
            {
                Timed t(c, st, kind_trunk, (uint64_t)n_rays * spr, timing);
                HIP_TRY(c, dt == NERF_MLP_BF16X3 ? nerf_trunk_seq_x3_launch(q, rgb_out != nullptr, c->n_cus, st)
                           : dt == NERF_MLP_F16X2 ? nerf_trunk_seq_f16x2_launch(q, rgb_out != nullptr, c->n_cus, st)
                           : dt == NERF_MLP_BF16  ? nerf_trunk_seq_bf16_launch(q, rgb_out != nullptr, c->n_cus, st)
                                                  : nerf_trunk_seq_launch(q, rgb_out != nullptr, c->n_cus, st));
                t.done(c->last_render);
            }
            if (rgb_out && dt != NERF_MLP_F32) {
                ColourArgs k{};
                k.wstream = stream_of(net, dt); k.small_params = net.small; k.live_count = ctr + 1; k.h8 = c->d_h8; k.slot_point = c->d_slot_point;
                k.ray_dirs = c->d_dirs; k.samples_per_ray = spr; k.rgb_out = rgb_out; k.nonfinite = split_dtype(dt) ? c->d_nonfinite : nullptr;
                Timed t(c, st, 4, 0, timing);
                HIP_TRY(c, dt == NERF_MLP_BF16X3 ? nerf_colour_x3_launch(k, c->n_cus, st)
                           : dt == NERF_MLP_F16X2 ? nerf_colour_f16x2_launch(k, c->n_cus, st)
                                                  : nerf_colour_bf16_launch(k, c->n_cus, st));
                t.done(c->last_render);
            }
            return NERF_OK;
        };
        MlpArgs a{};
        a.mode = MLP_MODE_RAYS;
        a.ray_dirs = c->d_dirs;
        a.origin[0] = cam->pos[0]; a.origin[1] = cam->pos[1]; a.origin[2] = cam->pos[2];
        // zero certification: 16-bit pre-activations of all samples -> plan (list 1, predicted cuts) -> exact kernel on list 1 -> audit ->
        // exact transmittance confirms the cuts (list 2 = what is left of the rays it does not) -> exact kernel on list 2
        auto cert_pass = [&](const DevNet &net, int which, int dt, int spr, const float *t_in, float *sigma_out, float *rgb_out, int kind) -> int {
            const int n_pts = n_rays * spr;
            unsigned int *slots = c->d_cert + kCertSlots * (2 * (size_t)passes + which);
            const unsigned cap = (unsigned)std::min<size_t>(cert_cap, (size_t)n_pts);
            // the pre-filter's arithmetic: f16 where the network fits its range (8 x closer to the exact pre-activations: tighter margins, a shorter
            // list), else bf16; a tile of the f16 pass that saw an activation leave the range counts in slots[12] and render_device goes back to bf16
            const bool pf16 = c->cert_prefilter_f16[which];
            const float *pf_stream = pf16 ? (const float *)net.wstream_f16v2 : stream_of(net, NERF_MLP_BF16);
            MlpArgs b = a;
            b.wstream = pf_stream; b.small_params = net.small; b.n_points = n_pts; b.samples_per_ray = spr; b.t = t_in;
            b.sigma_out = sigma_out; b.rgb_out = nullptr; b.raw_pre = 1; b.skip_empty = 0; b.skip_counter = nullptr; b.nonfinite = pf16 ? slots + 12 : nullptr;
            const int kind_side = which == 0 && !rgb_out ? 0 : 4;
            {
                Timed t(c, st, kind_side, 0, timing);
                if (c->cert_seq_prefilter) {
                    // the pre-filter walks each ray front to back and stops where its own (bf16) transmittance predicts the cut, a little
                    // later than k_cert_plan will (depth + 0.5): samples it never reaches stay NaN = "not evaluated" = uncertain
                    HIP_TRY(c, hipMemsetAsync(sigma_out, 0xFF, (size_t)n_pts * sizeof(float), st));
                    SeqArgs q{};
                    q.wstream = pf_stream; q.small_params = net.small; q.n_rays = n_rays; q.samples_per_ray = spr;
                    q.ray_dirs = c->d_dirs; q.t = t_in; q.far_ = cam->far_;
                    q.origin[0] = cam->pos[0]; q.origin[1] = cam->pos[1]; q.origin[2] = cam->pos[2];
                    q.sigma_out = sigma_out; q.ray_counter = slots + 8; q.stats = (unsigned long long *)(slots + 10);
                    q.prefilter = 1; q.prefilter_cut_T = expf(-(c->cert_depth_limit + 0.5f));
                    q.nonfinite = pf16 ? slots + 12 : nullptr;
                    HIP_TRY(c, pf16 ? nerf_trunk_seq_f16v2_launch(q, c->n_cus, st) : nerf_trunk_seq_bf16_launch(q, false, c->n_cus, st));
                } else HIP_TRY(c, pf16 ? nerf_mlp_f16v2_launch(b, c->n_cus, st) : launch_mlp(c, NERF_MLP_BF16, b, false, st));
                CertPlanArgs p{};
                p.pre = sigma_out; p.t = t_in; p.n_rays = n_rays; p.spr = spr; p.far_ = cam->far_;
                p.margin = c->cert_margin[which]; p.depth_limit = c->cert_depth_limit;
                p.audit_mask = c->cert_audit_mask; p.audit_mask_near = c->cert_audit_mask_near; p.audit_salt = (unsigned)(o->seed * 0x9E3779B97F4A7C15ull >> 32) + 0x632BE5ABu * passes + (unsigned)which;
                p.list = c->d_point_list; p.count = slots; p.capacity = cap; p.jstar = c->d_jstar;
                // full evaluations: probable zeros (pre-filter pre-activation below -margin x cert_zero_frac: several times the largest pre-filter error the lego audits see
                // is not needed for a skip -- a positive density among them only keeps its tile's colour heads) and the audited certificates go
                // to the back part of the list, whose all-zero tiles skip the colour head (exact: skip_empty)
                if (rgb_out && c->cert_zero_tiles) { p.count_back = slots + 9; p.zero_threshold = c->cert_margin[which] * c->cert_zero_frac; }
                p.aux = c->d_cert_aux; p.aux_count = slots + 7; p.aux_capacity = (unsigned)aux_cap;
                HIP_TRY(c, launch_cert_plan(p, st));
                if (rgb_out) HIP_TRY(c, hipMemsetAsync(rgb_out, 0, (size_t)n_pts * 3 * sizeof(float), st)); // weight 0 either way: 0 * 0
                t.done(c->last_render);
            }
            MlpArgs l = b;
            l.wstream = stream_of(net, dt); l.small_params = small_of(net, dt); zskip_of(c, net, l); l.raw_pre = 0; l.mode = MLP_MODE_LIST; l.rgb_out = rgb_out; l.n_points = (int)cap;
            l.point_list = c->d_point_list; l.point_list_count = slots;
            if (rgb_out && c->cert_zero_tiles) { l.point_list_count_back = slots + 9; l.skip_empty = 1; l.skip_counter = c->d_skip; }
            l.nonfinite = split_dtype(dt) ? c->d_nonfinite : nullptr;
            if (cap > 0) {
                // points = 0: the list's length is known on the device only (nerf_stats.n_exec_* report it after the frame)
                Timed t(c, st, kind, 0, timing);
                HIP_TRY(c, launch_mlp(c, dt, l, rgb_out != nullptr, st));
                t.done(c->last_render);
            }
            Timed t(c, st, kind_side, 0, timing);
            HIP_TRY(c, launch_cert_audit(c->d_cert_aux, slots + 7, (unsigned)aux_cap, sigma_out, slots + 2, c->n_cus, st));
            CertVerifyArgs v{};
            v.t = t_in; v.sigma = sigma_out; v.n_rays = n_rays; v.spr = spr; v.far_ = cam->far_; v.jstar = c->d_jstar;
            v.list = c->d_point_list; v.count = slots + 1; v.capacity = cap; v.fallback_rays = slots + 6;
            HIP_TRY(c, launch_cert_verify(v, st));
            l.point_list_count = slots + 1; l.point_list_count_back = nullptr;
            if (cap > 0) HIP_TRY(c, launch_mlp(c, dt, l, rgb_out != nullptr, st)); // usually an empty list: the launch returns at once
            t.done(c->last_render);
            return NERF_OK;
        };
        // coarse network: sigma only unless its colours are composited (reference discards them, src/lib.rs:404)
        a.wstream = stream_of(NC, dtype_coarse); a.small_params = small_of(NC, dtype_coarse); zskip_of(c, NC, a);
        a.n_points = n_rays * nc; a.samples_per_ray = nc; a.t = c->d_tc;
        a.sigma_out = c->d_sc; a.rgb_out = o->coarse_only ? c->d_rgbc : nullptr; // sigma-only launch otherwise
        a.skip_empty = o->skip_empty; a.skip_counter = o->skip_empty ? c->d_skip : nullptr; // only full kernels look at it
        a.nonfinite = split_dtype(dtype_coarse) ? c->d_nonfinite : nullptr;
        if (seq) {
            if ((rc = seq_pass(NC, dtype_coarse, nc, c->d_tc, c->d_sc, o->coarse_only ? c->d_rgbc : nullptr, 3 * (int)passes, o->coarse_only ? 1 : 0))) return rc;
        } else if (certify) {
            if ((rc = cert_pass(NC, 0, dtype_coarse, nc, c->d_tc, c->d_sc, o->coarse_only ? c->d_rgbc : nullptr, o->coarse_only ? 1 : 0))) return rc;
        } else {
            Timed t(c, st, o->coarse_only ? 1 : 0, (uint64_t)a.n_points, timing);
            HIP_TRY(c, launch_mlp(c, dtype_coarse, a, o->coarse_only != 0, st));
            t.done(c->last_render);
        }
        float *pass_out = ray_out + (size_t)row * RW * 3;
        CompositeArgs ca{};
        ca.n_rays = n_rays; ca.far_ = cam->far_; ca.out = pass_out;
        ca.depth = ray_depth ? ray_depth + (size_t)row * RW : nullptr;
        ca.opacity = ray_opacity ? ray_opacity + (size_t)row * RW : nullptr;
        if (background) { ca.use_bg = 1; ca.bg[0] = background[0]; ca.bg[1] = background[1]; ca.bg[2] = background[2]; }
        if (o->coarse_only) {
            ca.n = nc; ca.t = c->d_tc; ca.sigma = c->d_sc; ca.rgb = c->d_rgbc;
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_composite(ca, st));
            t.done(c->last_render);
            continue;
        }
        const float *t_fine = c->d_tc;
        if (nf > 0) {
            ResampleArgs ra{};
            ra.g = g; ra.n_rays = n_rays; ra.nc = nc; ra.nf = nf; ra.far_ = cam->far_;
            ra.seed_lo = (uint32_t)o->seed; ra.seed_hi = (uint32_t)(o->seed >> 32);
            ra.t_coarse = c->d_tc; ra.sigma_coarse = c->d_sc; ra.t_fine = c->d_tf;
            unsigned int *hctr = seq ? c->d_seq + 4 * (size_t)(3 * passes + 2) : nullptr; // {queue head, flagged-ray count, u64 chunks}
            if (hybrid) { ra.flag_tau = c->hybrid_tau; ra.flag_count = hctr + 1; ra.flag_list = c->d_flag_list; }
            {
                Timed t(c, st, 2, 0, timing);
                HIP_TRY(c, launch_resample(ra, st));
                t.done(c->last_render);
            }
            if (hybrid) {
                // The coarse densities came from the split arithmetic.  Redo, in exact f32, the rays with a draw in a light CDF
                // bin (their sample positions are the ill-conditioned ones) and resample just those: same positions as the f32 path.
                SeqArgs q{};
                q.wstream = NC.wstream; q.small_params = NC.small_f32; zskip_of(c, NC, q); q.n_rays = n_rays; q.samples_per_ray = nc;
                q.ray_dirs = c->d_dirs; q.t = c->d_tc; q.far_ = cam->far_;
                q.origin[0] = cam->pos[0]; q.origin[1] = cam->pos[1]; q.origin[2] = cam->pos[2];
                q.sigma_out = c->d_sc; q.ray_counter = hctr; q.stats = (unsigned long long *)(hctr + 2);
                q.live_count = nullptr; // hctr[1] is the LENGTH of the ray list below: this launch never exports (no colour head)
                q.ray_list = c->d_flag_list; q.ray_list_count = hctr + 1; q.zero_fill_after_cut = 1;
                {
                    Timed t(c, st, 0, 0, timing);
                    HIP_TRY(c, nerf_trunk_seq_launch(q, false, c->n_cus, st));
                    t.done(c->last_render);
                }
                ResampleArgs rb = ra;
                rb.flag_tau = 0.0f; rb.flag_count = nullptr; rb.flag_list = nullptr;
                rb.ray_list = c->d_flag_list; rb.ray_list_count = hctr + 1;
                Timed t(c, st, 2, 0, timing);
                HIP_TRY(c, launch_resample(rb, st));
                t.done(c->last_render);
            }
            t_fine = c->d_tf;
        }
        a.wstream = stream_of(NF, dtype); a.small_params = small_of(NF, dtype); zskip_of(c, NF, a);
        a.n_points = n_rays * M; a.samples_per_ray = M; a.t = t_fine;
        a.sigma_out = c->d_sf; a.rgb_out = c->d_rgbf;
        a.clock_out = c->d_clock; // NULL unless NERF_DEBUG_CLOCK=1
        a.nonfinite = split_dtype(dtype) ? c->d_nonfinite : nullptr;
        c->clock_valid = c->d_clock != nullptr;
        if (seq) {
            if ((rc = seq_pass(NF, dtype, M, t_fine, c->d_sf, c->d_rgbf, 3 * (int)passes + 1, 1))) return rc;
        } else if (certify) {
            if ((rc = cert_pass(NF, 1, dtype, M, t_fine, c->d_sf, c->d_rgbf, 1))) return rc;
        } else {
            Timed t(c, st, 1, (uint64_t)a.n_points, timing);
            HIP_TRY(c, launch_mlp(c, dtype, a, true, st));
            t.done(c->last_render);
        }
        ca.n = M; ca.t = t_fine; ca.sigma = c->d_sf; ca.rgb = c->d_rgbf;
        {
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_composite(ca, st));
            t.done(c->last_render);
        }
    }
    if (s > 1) {
        Timed t(c, st, 2, 0, timing);
        HIP_TRY(c, launch_box_downsample(c->d_rayfb, d_out, cw, ch, s, 3, st));
        if (d_depth) HIP_TRY(c, launch_box_downsample(ray_depth, d_depth, cw, ch, s, 1, st));
        if (d_opacity) HIP_TRY(c, launch_box_downsample(ray_opacity, d_opacity, cw, ch, s, 1, st));
        t.done(c->last_render);
    }
    // the dominant-kernel events also feed nerf_kernel_time_query (ownership: see recycle_render)
    for (const auto &p : c->last_render)
        if (p.kind == 1) c->dominant.push_back(p);
    scope.ok = true;
    if (cert) { // the audit's outcome decides whether this frame stands (render_device): certify_zero renders synchronise the stream
        HIP_TRY(c, hipStreamSynchronize(st));
        std::vector<unsigned int> h((size_t)passes * 2 * kCertSlots);
        HIP_TRY(c, hipMemcpy(h.data(), c->d_cert, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < passes * 2; ++k) {
            const unsigned int *q = &h[(size_t)k * kCertSlots];
            const int w = (int)(k & 1);
            if (w == 1 && o->coarse_only) continue;
            cert->used[w] = true;
            cert->listed[w] += std::min<uint64_t>((uint64_t)q[0] + q[9], cert->list_capacity) + std::min<uint64_t>(q[1], cert->list_capacity);
            cert->list_need = std::max<uint64_t>(cert->list_need, std::max<uint64_t>((uint64_t)q[0] + q[9], q[1]));
            cert->audited[w] += q[2]; cert->violations[w] += q[3];
            if (q[2]) {
                const unsigned bits = 0x7f800000u - q[4];
                float hr, er;
                memcpy(&hr, &bits, sizeof hr); memcpy(&er, &q[5], sizeof er);
                cert->headroom[w] = std::min(cert->headroom[w], hr); cert->max_err[w] = std::max(cert->max_err[w], er);
            }
            cert->fallback_rays += q[6];
            cert->range_left[w] += q[12];
        }
    }
    if (stats) {
        HIP_TRY(c, hipStreamSynchronize(st));
        memset(stats, 0, sizeof *stats);
        stats->n_rays = (uint64_t)RW * RH;
        stats->n_passes = passes;
        stats->n_coarse_points = stats->n_rays * (uint64_t)nc;                       // nominal: every sample of every ray
        stats->n_fine_points = o->coarse_only ? 0 : stats->n_rays * (uint64_t)M;
        for (const auto &p : c->last_render) {
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, p.a, p.b));
            if (p.kind == 0) { stats->ms_coarse_mlp += ms; stats->n_mlp_launches++; }
            else if (p.kind == 1) {
                stats->n_mlp_launches++;
                if (o->coarse_only) stats->ms_coarse_mlp += ms; else stats->ms_fine_mlp += ms;
            } else if (p.kind == 4) { // colour head on the compacted live samples (skip_dead)
                stats->n_mlp_launches++;
                if (o->coarse_only) stats->ms_coarse_mlp += ms; else stats->ms_fine_mlp += ms;
            } else stats->ms_other += ms;
        }
        if (!c->last_render.empty()) {
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->last_render.front().a, c->last_render.back().b));
            stats->ms_total = ms;
        }
        if (watch_range) {
            unsigned int bad = 0;
            HIP_TRY(c, hipMemcpy(&bad, c->d_nonfinite, sizeof bad, hipMemcpyDeviceToHost));
            stats->n_nonfinite_points = bad;
        }
        if ((o->skip_empty || certify) && c->d_skip) { // certify_zero: all-zero tiles of the list's back part (probable zeros, audited certificates)
            unsigned long long tiles = 0;
            HIP_TRY(c, hipMemcpy(&tiles, c->d_skip, sizeof tiles, hipMemcpyDeviceToHost));
            stats->n_colour_skipped_points = (uint64_t)tiles * nerfmlp::kPointsPerBlock;
        }
        // evaluations actually executed
        stats->n_exec_coarse_trunk = stats->n_coarse_points;
        stats->n_exec_fine_trunk = stats->n_fine_points;
        stats->n_exec_colour = (o->coarse_only ? stats->n_coarse_points : stats->n_fine_points) - stats->n_colour_skipped_points;
        if (certify && cert) { // samples the exact kernel evaluated = the lengths of the lists (audited certificates included)
            stats->n_exec_coarse_trunk = cert->listed[0];
            stats->n_exec_fine_trunk = o->coarse_only ? 0 : cert->listed[1];
            stats->n_exec_colour = (o->coarse_only ? cert->listed[0] : cert->listed[1]) - std::min<uint64_t>(stats->n_colour_skipped_points, o->coarse_only ? cert->listed[0] : cert->listed[1]);
            stats->n_certify_audited = cert->audited[0] + cert->audited[1];
            stats->n_certify_violations = cert->violations[0] + cert->violations[1];
            stats->n_certify_fallback_rays = (uint32_t)std::min<uint64_t>(cert->fallback_rays, 0xffffffffu);
            for (int w = 0; w < 2; ++w) { stats->certify_margin[w] = c->cert_margin[w]; stats->certify_headroom[w] = cert->headroom[w]; stats->certify_max_error[w] = cert->max_err[w]; }
        }
        if (seq) {
            std::vector<unsigned int> h((size_t)passes * 3 * 4);
            HIP_TRY(c, hipMemcpy(h.data(), c->d_seq, h.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
            uint64_t evaluated[3] = {0, 0, 0}, live = 0; // samples the trunk launches evaluated (a ray's last chunk may be partial)
            for (uint32_t k = 0; k < passes * 3; ++k) {
                unsigned long long ch64;
                memcpy(&ch64, &h[4 * (size_t)k + 2], sizeof ch64);
                evaluated[k % 3] += ch64;
                if (k % 3 == 2) stats->n_hybrid_rays += h[4 * (size_t)k + 1]; // flagged rays redone in f32
                else live += h[4 * (size_t)k + 1];
            }
            stats->n_exec_coarse_trunk = evaluated[0] + evaluated[2];
            stats->n_exec_fine_trunk = o->coarse_only ? 0 : evaluated[1];
            stats->n_exec_colour = live;
            stats->n_colour_skipped_points = (o->coarse_only ? stats->n_coarse_points : stats->n_fine_points) - live;
        }
        if (stats->n_nonfinite_points) { // the frame is WRONG there (f16 overflow yields finite garbage, not NaN): never return it as a success
            char msg[320];
            snprintf(msg, sizeof msg, "%llu evaluations: an operand left the range of the split arithmetic (NERF_MLP_F16X2: |activation| <= 65504) or a "
                     "density was not finite; the frame is not usable -- use NERF_MLP_BF16X3 or NERF_MLP_F32", (unsigned long long)stats->n_nonfinite_points);
            return fail(c, NERF_ERR_STATE, msg);
        }
    }
    return NERF_OK;
}


// ---- ray batches (nerf_render_rays) -------------------------------------------------------------------------------------
// What the header's contract needs beside render_once: the rays are the caller's, so there is no camera, no window and none of the modes
// tied to either.  Per pass of at most max_rays_per_pass rays (rays * samples <= 0x3fffffff, as above):
//     k_batch_prepare -> coarse MLP (sigma) -> resample/sort -> fine MLP -> composite
// A shared origin runs the image path's MLP_MODE_RAYS launches (the origin rides in the kernel arguments); per-ray origins expand every
// pass's samples into points + per-sample directions (k_batch_points, 24 B per sample in c->d_batch) for MLP_MODE_POINTS, which forms
// nothing itself and then runs the same per-column arithmetic: the two paths carry the same bits.
struct RayBatch {
    const float *h_origin;     // n_origins == 1: the shared origin (HOST, 3 floats); else NULL
    const float *d_origins;    // n_origins == n_rays: n_rays x 3 (device); else NULL
    const float *d_dirs;       // n_rays x 3 (device)
    size_t n_rays;
    int normalize;
    float near_, far_;
    const float *d_bounds;     // n_rays x 2 (device) or NULL
    const uint32_t *d_rng;     // n_rays (device) or NULL
};

// everything nerf_render_rays* can refuse without a context or a device, in the header's order
int check_ray_batch(nerf_ctx *c, const void *origins, size_t n_origins, const void *dirs, size_t n_rays, float near_, float far_, const void *bounds,
                    const nerf_render_opts *o, const float *background, const void *rgb_out) {
    if (!o) return fail(c, NERF_ERR_INVALID, "opts is NULL");
    if (n_rays > (size_t)0x7fffffff) return fail(c, NERF_ERR_INVALID, "n_rays must be at most INT32_MAX");
    if (n_rays > 0 && (!origins || !dirs || !rgb_out)) return fail(c, NERF_ERR_INVALID, "origins, dirs and rgb_out must not be NULL");
    if (n_origins != 1 && n_origins != n_rays) return fail(c, NERF_ERR_INVALID, "n_origins must be 1 (one origin for every ray) or n_rays");
    if (o->crop_x0 || o->crop_y0 || o->crop_w || o->crop_h) return fail(c, NERF_ERR_INVALID, "ray batches have no pixel grid: crop_* must be 0");
    if (o->ssaa > 1) return fail(c, NERF_ERR_INVALID, "ray batches have no pixel grid: ssaa must be 0 or 1");
    if (o->band_count > 1) return fail(c, NERF_ERR_INVALID, "ray batches have no rows: band_count must be 0 or 1");
    if (o->skip_empty || o->skip_dead || o->hybrid_sampling || o->certify_zero)
        return fail(c, NERF_ERR_INVALID, "skip_empty, skip_dead, hybrid_sampling and certify_zero are not available for ray batches (first version)");
    if (o->n_coarse <= 0) return fail(c, NERF_ERR_INVALID, "coarse samples per ray must be greater than 0");
    if (o->n_fine < 0) return fail(c, NERF_ERR_INVALID, "fine samples per ray must be >= 0");
    if (!valid_dtype(o->mlp_dtype)) return fail(c, NERF_ERR_INVALID, "mlp_dtype must be NERF_MLP_F32, NERF_MLP_BF16, NERF_MLP_BF16X3 or NERF_MLP_F16X2");
    if (!bounds) {
        if (!std::isfinite(near_) || !std::isfinite(far_)) return fail(c, NERF_ERR_INVALID, "near_ and far_ must be finite when bounds is NULL");
        if (!(far_ > near_)) return fail(c, NERF_ERR_INVALID, "far_ must be greater than near_ when bounds is NULL");
    }
    if (background && !(std::isfinite(background[0]) && std::isfinite(background[1]) && std::isfinite(background[2])))
        return fail(c, NERF_ERR_INVALID, "background components must be finite");
    const int nc = o->n_coarse, nf = (o->coarse_only || o->n_fine == 0 || nc < 3) ? 0 : o->n_fine;
    if ((long long)nc + nf > 0x3fffffff || composite_lds_bytes(nc + nf) > 160 * 1024 || (nf > 0 && resample_lds_bytes(nc, nf) > 160 * 1024))
        return fail(c, NERF_ERR_INVALID, "too many samples per ray for the sampling / compositing kernels (one ray per wave in LDS)");
    return NERF_OK;
}

// the host entry point's per-ray checks: the first offending ray is named
int check_ray_batch_rays(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, const float *bounds) {
    char msg[160];
    auto finite3 = [](const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    for (size_t r = 0; r < n_rays; ++r) {
        const char *what = nullptr;
        const float *d = dirs + 3 * r;
        if (r < n_origins && !finite3(origins + 3 * r)) what = "its origin is not finite";
        else if (!finite3(d)) what = "its direction is not finite";
        else if (normalize && d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) what = "its direction is zero and cannot be normalised";
        else if (bounds && !(std::isfinite(bounds[2 * r]) && std::isfinite(bounds[2 * r + 1]))) what = "its bounds are not finite";
        else if (bounds && !(bounds[2 * r + 1] > bounds[2 * r])) what = "its far is not greater than its near";
        if (what) {
            snprintf(msg, sizeof msg, "ray %zu: %s", r, what);
            return fail(c, NERF_ERR_INVALID, msg);
        }
    }
    return NERF_OK;
}

// what nerf_render_rays_normals* adds to check_ray_batch
int check_normals(nerf_ctx *c, float h, const void *normals_out) {
    if (!(std::isfinite(h) && h > 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and greater than 0");
    if (!normals_out) return fail(c, NERF_ERR_INVALID, "normals_out must not be NULL");
    return NERF_OK;
}

// largest batch of nerf_forward_batch*: INT32_MAX minus (persistent workgroups + 1) tiles of the widest kernel (256 points)
size_t max_batch_points(int n_cus) { return (size_t)0x7fffffff - ((size_t)n_cus + 1) * 256; }

// the f32 sigma-only MLP_MODE_POINTS launch (nerf_density_batch's) over n points
hipError_t launch_sigma_points(const nerf_ctx *c, const DevNet &net, const float *d_pts, size_t n, float *d_sigma, hipStream_t st) {
    MlpArgs a{};
    a.mode = MLP_MODE_POINTS;
    a.wstream = net.wstream; a.small_params = net.small_f32; zskip_of(c, net, a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.sigma_out = d_sigma;
    return launch_mlp(c, NERF_MLP_F32, a, false, st);
}

// The pass workspace of a normals render in c->d_normal, every part 256-byte aligned.
struct NormalWorkspace {
    float *w; uint32_t *list, *count, *base, *bsum, *totals;
    static size_t al(size_t bytes) { return (bytes + 255) / 256 * 256; }
    static size_t blocks(size_t rays) { return (rays + kNormalBlock - 1) / kNormalBlock; }
    static size_t bytes(size_t rays, size_t samples) { return 2 * al(4 * samples) + 2 * al(4 * rays) + al(4 * blocks(rays)) + 256; }
    NormalWorkspace(void *p, size_t rays, size_t samples) {
        char *q = (char *)p;
        w = (float *)q; q += al(4 * samples);
        list = (uint32_t *)q; q += al(4 * samples);
        count = (uint32_t *)q; q += al(4 * rays);
        base = (uint32_t *)q; q += al(4 * rays);
        bsum = (uint32_t *)q; q += al(4 * blocks(rays));
        totals = (uint32_t *)q;
    }
};

// arguments already checked (check_ray_batch, check_normals); asynchronous on st unless stats != NULL.
// d_normals != NULL (n_rays x 3): the compositing launch also hands out its weights, and per pass
//     count + scan + list (3 launches) -> [8 bytes to the host] -> stencil -> sigma-only MLP over 6 L points -> reduce
// follow.  The live total L of a pass goes back to the host -- ONE SMALL COPY AND ONE STREAM SYNCHRONISATION PER PASS, as mesh_extract reads
// its counts: it sizes the stencil workspace (16 B per point, grown on demand) and the launches that follow; a pass with L = 0 launches
// nothing further and writes zero normals.  The network differentiated is the one composited, always in f32.
int render_rays_device(nerf_ctx *c, const RayBatch &b, const nerf_render_opts *o, const float *background, float *d_out, float *d_depth,
                       float *d_opacity, hipStream_t st, nerf_stats *stats, float h = 0.0f, float *d_normals = nullptr) {
    int rc;
    const int dtype = o->mlp_dtype;
    const int dtype_coarse = (split_dtype(dtype) && !o->coarse_only) ? NERF_MLP_F32 : dtype; // as render_once: the sampling pass stays in exact f32
    if (!c->net[NERF_NET_COARSE].loaded) return fail(c, NERF_ERR_STATE, "coarse network not loaded");
    if (!o->coarse_only && !c->net[NERF_NET_FINE].loaded) return fail(c, NERF_ERR_STATE, "fine network not loaded");
    if (dtype == NERF_MLP_F16X2 && !c->net[o->coarse_only ? NERF_NET_COARSE : NERF_NET_FINE].wstream_x2)
        return fail(c, NERF_ERR_STATE, "NERF_MLP_F16X2 is unavailable for this network: a weight exceeds the f16 range");
    const int nc = o->n_coarse;
    const int nf = (o->coarse_only || o->n_fine == 0 || nc < 3) ? 0 : o->n_fine; // the sample-count branches of render_once
    const int M = nc + nf;
    size_t pass_cap = std::max<size_t>(1, std::min<size_t>(c->max_rays_per_pass, (size_t)0x3fffffff / (size_t)M));
    // normals: if every sample of a pass were live its 6 stencil points each must still fit one MLP launch
    if (d_normals) pass_cap = std::max<size_t>(1, std::min<size_t>(pass_cap, max_batch_points(c->n_cus) / (6 * (size_t)M)));
    const size_t pass_rays = std::min(b.n_rays, pass_cap);
    if ((rc = ensure_workspace(c, pass_rays, nc, M, o->coarse_only != 0))) return rc;
    const int n_comp = o->coarse_only ? nc : M; // samples per ray that the final compositing integrates
    if (d_normals && (rc = ensure_bytes(c, &c->d_normal, &c->normal_bytes, NormalWorkspace::bytes(pass_rays, pass_rays * (size_t)n_comp)))) return rc;
    const NormalWorkspace nw(c->d_normal, pass_rays, pass_rays * (size_t)n_comp);
    c->normal_live = 0; c->normal_samples = 0;
    // c->d_batch (floats): [far per ray, padded to 64][points 3 x n SoA][directions n x 3 AoS], n = the pass's rays x M
    const bool expand = b.d_origins != nullptr;
    const size_t far_floats = b.d_bounds ? (pass_rays + 63) / 64 * 64 : 0, n_max = pass_rays * (size_t)M;
    float *d_far = nullptr, *d_pts = nullptr, *d_daos = nullptr;
    if (far_floats || expand) {
        if ((rc = ensure_bytes(c, &c->d_batch, &c->batch_bytes, (far_floats + (expand ? 6 * n_max : 0)) * sizeof(float)))) return rc;
        d_far = b.d_bounds ? (float *)c->d_batch : nullptr;
        d_pts = (float *)c->d_batch + far_floats; d_daos = d_pts + 3 * n_max;
    }
    // events: all owned by last_render (kind 5, not 1, for the colour-producing network: c->dominant and with it nerf_kernel_time_query
    // belong to image renders)
    recycle_render(c);
    const bool watch_range = c->d_nonfinite && (split_dtype(dtype) || split_dtype(dtype_coarse));
    if (watch_range) HIP_TRY(c, hipMemsetAsync(c->d_nonfinite, 0, sizeof(unsigned int), st));
    const bool timing = true;
    const DevNet &NC = c->net[NERF_NET_COARSE], &NF = c->net[NERF_NET_FINE];
    uint32_t passes = 0;
    for (size_t r0 = 0; r0 < b.n_rays; r0 += pass_cap, ++passes) {
        const int n_rays = (int)std::min(pass_cap, b.n_rays - r0);
        const float *far_per_ray = d_far;
        const float *origins = expand ? b.d_origins + 3 * r0 : nullptr;
        {
            BatchPrepareArgs p{};
            p.n_rays = n_rays; p.first_ray = (uint32_t)r0; p.dirs = b.d_dirs + 3 * r0; p.normalize = b.normalize;
            p.bounds = b.d_bounds ? b.d_bounds + 2 * r0 : nullptr; p.rng_index = b.d_rng ? b.d_rng + r0 : nullptr;
            p.near_ = b.near_; p.far_ = b.far_; p.count = nc; p.seed_lo = (uint32_t)o->seed; p.seed_hi = (uint32_t)(o->seed >> 32);
            p.dirs_out = c->d_dirs; p.t_out = c->d_tc; p.far_out = d_far;
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_batch_prepare(p, st));
            t.done(c->last_render);
        }
        // the normals of the pass, from the weights the compositing launch left in nw.w (t: the composited samples' positions)
        auto normals_pass = [&](const DevNet &net, const float *t) -> int {
            if (!d_normals) return NERF_OK;
            NormalListArgs la{nw.w, n_rays, n_comp, nw.count, nw.base, nw.bsum, nw.totals, nw.list};
            {
                Timed tm(c, st, 7, 0, timing);
                HIP_TRY(c, launch_normal_list(la, st));
                tm.done(c->last_render);
            }
            uint32_t totals[2] = {0, 0};
            HIP_TRY(c, hipMemcpyAsync(totals, nw.totals, sizeof totals, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            const size_t L = totals[0];
            c->normal_live += L; c->normal_samples += (uint64_t)n_rays * (uint64_t)n_comp;
            float *out = d_normals + 3 * r0;
            if (L == 0) { HIP_TRY(c, hipMemsetAsync(out, 0, (size_t)n_rays * 3 * sizeof(float), st)); return NERF_OK; }
            if (L > (size_t)n_rays * (size_t)n_comp) return fail(c, NERF_ERR_HIP, "normals: the live count exceeds the pass's samples");
            int rc2;
            if ((rc2 = ensure_bytes(c, &c->d_stencil, &c->stencil_bytes, 6 * L * 4 * sizeof(float)))) return rc2;
            float *d_spts = (float *)c->d_stencil, *d_ssig = d_spts + 18 * L;
            NormalStencilArgs sa{};
            sa.n_live = (uint32_t)L; sa.h = h; sa.list = nw.list; sa.spr = n_comp; sa.origins = origins; sa.dirs = c->d_dirs; sa.t = t; sa.pts = d_spts;
            if (!expand) { sa.origin[0] = b.h_origin[0]; sa.origin[1] = b.h_origin[1]; sa.origin[2] = b.h_origin[2]; }
            {
                Timed tm(c, st, 7, 0, timing);
                HIP_TRY(c, launch_normal_stencil(sa, st));
                tm.done(c->last_render);
            }
            {
                Timed tm(c, st, 6, (uint64_t)(6 * L), timing);
                HIP_TRY(c, launch_sigma_points(c, net, d_spts, 6 * L, d_ssig, st));
                tm.done(c->last_render);
            }
            NormalReduceArgs ra{n_rays, (uint32_t)L, nw.count, nw.base, nw.list, nw.w, d_spts, d_ssig, out};
            Timed tm(c, st, 7, 0, timing);
            HIP_TRY(c, launch_normal_reduce(ra, st));
            tm.done(c->last_render);
            return NERF_OK;
        };
        MlpArgs a{};
        a.ray_dirs = c->d_dirs;
        if (expand) a.mode = MLP_MODE_POINTS;
        else { a.mode = MLP_MODE_RAYS; a.origin[0] = b.h_origin[0]; a.origin[1] = b.h_origin[1]; a.origin[2] = b.h_origin[2]; }
        // per-ray origins: the points and per-sample directions of the launch that follows (a.n_points, a.t, a.samples_per_ray are set)
        auto expand_points = [&]() -> int {
            if (!expand) return NERF_OK;
            BatchPointsArgs q{};
            q.n_rays = n_rays; q.spr = a.samples_per_ray; q.origins = origins; q.dirs = c->d_dirs; q.t = a.t;
            q.pts_soa = d_pts; q.dirs_aos = d_daos;
            a.pts_soa = d_pts; a.dirs_aos = d_daos;
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_batch_points(q, st));
            t.done(c->last_render);
            return NERF_OK;
        };
        a.wstream = stream_of(NC, dtype_coarse); a.small_params = small_of(NC, dtype_coarse); zskip_of(c, NC, a);
        a.n_points = n_rays * nc; a.samples_per_ray = nc; a.t = c->d_tc;
        a.sigma_out = c->d_sc; a.rgb_out = o->coarse_only ? c->d_rgbc : nullptr;
        a.nonfinite = split_dtype(dtype_coarse) ? c->d_nonfinite : nullptr;
        // only the f32 kernel has a sigma-only points mode: a bf16 sampling pass over expanded points runs the full kernel (the same
        // densities) and leaves its colours in the fine pass's buffer, which that pass overwrites
        bool full_coarse = o->coarse_only != 0;
        if (expand && !full_coarse && dtype_coarse != NERF_MLP_F32) { full_coarse = true; a.rgb_out = c->d_rgbf; }
        if ((rc = expand_points())) return rc;
        {
            Timed t(c, st, o->coarse_only ? 5 : 0, (uint64_t)a.n_points, timing);
            HIP_TRY(c, launch_mlp(c, dtype_coarse, a, full_coarse, st));
            t.done(c->last_render);
        }
        CompositeArgs ca{};
        ca.n_rays = n_rays; ca.far_ = b.far_; ca.far_per_ray = far_per_ray; ca.out = d_out + 3 * r0;
        ca.depth = d_depth ? d_depth + r0 : nullptr; ca.opacity = d_opacity ? d_opacity + r0 : nullptr;
        if (background) { ca.use_bg = 1; ca.bg[0] = background[0]; ca.bg[1] = background[1]; ca.bg[2] = background[2]; }
        if (d_normals) ca.w_out = nw.w;
        if (o->coarse_only) {
            ca.n = nc; ca.t = c->d_tc; ca.sigma = c->d_sc; ca.rgb = c->d_rgbc;
            {
                Timed t(c, st, 2, 0, timing);
                HIP_TRY(c, launch_composite(ca, st));
                t.done(c->last_render);
            }
            if ((rc = normals_pass(NC, c->d_tc))) return rc;
            continue;
        }
        const float *t_fine = c->d_tc;
        if (nf > 0) {
            ResampleArgs ra{};
            ra.n_rays = n_rays; ra.nc = nc; ra.nf = nf; ra.far_ = b.far_; ra.far_per_ray = far_per_ray;
            ra.seed_lo = (uint32_t)o->seed; ra.seed_hi = (uint32_t)(o->seed >> 32);
            ra.t_coarse = c->d_tc; ra.sigma_coarse = c->d_sc; ra.t_fine = c->d_tf;
            // the index of Philox stream 1: the caller's, or the ray's number in the batch -- a one-row rectangle that starts at column r0
            ra.pixel_index = b.d_rng ? b.d_rng + r0 : nullptr;
            ra.g.n_rays = n_rays; ra.g.rx0 = (int)r0; ra.g.ry0 = 0; ra.g.rw = n_rays; ra.g.rnx = n_rays; ra.g.rny = 1;
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_resample(ra, st));
            t.done(c->last_render);
            t_fine = c->d_tf;
        }
        a.wstream = stream_of(NF, dtype); a.small_params = small_of(NF, dtype); zskip_of(c, NF, a);
        a.n_points = n_rays * M; a.samples_per_ray = M; a.t = t_fine;
        a.sigma_out = c->d_sf; a.rgb_out = c->d_rgbf;
        a.nonfinite = split_dtype(dtype) ? c->d_nonfinite : nullptr;
        if ((rc = expand_points())) return rc;
        {
            Timed t(c, st, 5, (uint64_t)a.n_points, timing);
            HIP_TRY(c, launch_mlp(c, dtype, a, true, st));
            t.done(c->last_render);
        }
        ca.n = M; ca.t = t_fine; ca.sigma = c->d_sf; ca.rgb = c->d_rgbf;
        {
            Timed t(c, st, 2, 0, timing);
            HIP_TRY(c, launch_composite(ca, st));
            t.done(c->last_render);
        }
        if ((rc = normals_pass(NF, t_fine))) return rc;
    }
    if (stats) {
        HIP_TRY(c, hipStreamSynchronize(st));
        memset(stats, 0, sizeof *stats);
        stats->n_rays = b.n_rays;
        stats->n_passes = passes;
        stats->n_coarse_points = stats->n_rays * (uint64_t)nc;
        stats->n_fine_points = o->coarse_only ? 0 : stats->n_rays * (uint64_t)M;
        double ms_normal_sigma = 0.0, ms_normal_small = 0.0;
        for (const auto &p : c->last_render) {
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, p.a, p.b));
            if (p.kind == 0) { stats->ms_coarse_mlp += ms; stats->n_mlp_launches++; }
            else if (p.kind == 5) {
                stats->n_mlp_launches++;
                if (o->coarse_only) stats->ms_coarse_mlp += ms; else stats->ms_fine_mlp += ms;
            } else stats->ms_other += ms; // kinds 6 and 7 too: a normals render's own launches are neither network pass of the colour
            if (p.kind == 6) ms_normal_sigma += ms; else if (p.kind == 7) ms_normal_small += ms;
        }
        if (!c->last_render.empty()) {
            float ms = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&ms, c->last_render.front().a, c->last_render.back().b));
            stats->ms_total = ms;
        }
        if (d_normals && c->debug_normals)
            fprintf(stderr, "nerf normals: %llu live of %llu composited samples, sigma launches %.3f ms over %llu points, other normal kernels %.3f ms\n",
                    (unsigned long long)c->normal_live, (unsigned long long)c->normal_samples, ms_normal_sigma, (unsigned long long)(6 * c->normal_live),
                    ms_normal_small);
        if (watch_range) {
            unsigned int bad = 0;
            HIP_TRY(c, hipMemcpy(&bad, c->d_nonfinite, sizeof bad, hipMemcpyDeviceToHost));
            stats->n_nonfinite_points = bad;
        }
        stats->n_exec_coarse_trunk = stats->n_coarse_points;
        stats->n_exec_fine_trunk = stats->n_fine_points;
        stats->n_exec_colour = o->coarse_only ? stats->n_coarse_points : stats->n_fine_points;
        if (stats->n_nonfinite_points) { // as an image render: never returned as a success
            char msg[320];
            snprintf(msg, sizeof msg, "%llu evaluations: an operand left the range of the split arithmetic (NERF_MLP_F16X2: |activation| <= 65504) or a "
                     "density was not finite; the batch is not usable -- use NERF_MLP_BF16X3 or NERF_MLP_F32", (unsigned long long)stats->n_nonfinite_points);
            return fail(c, NERF_ERR_STATE, msg);
        }
    }
    return NERF_OK;
}

} // namespace

// certify_zero frames are AUDITED (k_cert_audit: 1 in 16 of the samples certified by less than twice the margin and 1 in 128 of the others are evaluated exactly all the same).  A frame stands only if no
// audited certificate was wrong and the closest audited sample kept at least half the margin between itself and a positive density;
// otherwise the network's margin is widened -- for good: c->cert_margin is per context and network, reset when a network is loaded --
// and the frame is rendered again.  The same loop grows the sample list when a pass wanted more entries than it had.  Margins are
// measurements, not proofs: what this buys is that a network on which bf16 is less accurate than on the lego scene
// calibrates itself or fails loudly (NERF_ERR_STATE) instead of returning a silently different frame.
// Every attempt writes the whole frame -- colour and the requested maps -- so the maps returned are those of the frame that stands.
int nerfint::render_device(nerf_ctx *c, const nerf_camera *cam, const nerf_render_opts *o, float *d_out, float *d_depth, float *d_opacity,
                           hipStream_t st, nerf_stats *stats, const float *background) {
    if (!o || !o->certify_zero) return render_once(c, cam, o, d_out, d_depth, d_opacity, st, stats, nullptr, background);
    constexpr int kMaxRetries = 8;
    uint64_t violations = 0;
    for (int attempt = 0;; ++attempt) {
        CertOutcome oc;
        const int rc = render_once(c, cam, o, d_out, d_depth, d_opacity, st, stats, &oc, background);
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
        if (stats) { stats->n_certify_retries = (uint32_t)attempt; stats->n_certify_violations = violations; }
        if (!again) return NERF_OK;
        if (attempt == kMaxRetries) {
            char msg[320];
            snprintf(msg, sizeof msg, "certify_zero: %s after %d renders of this frame (margins now %g / %g): the 16-bit pass cannot certify this network's "
                     "zero densities; render with certify_zero = 0", why.c_str(), attempt + 1, (double)c->cert_margin[0], (double)c->cert_margin[1]);
            return fail(c, NERF_ERR_STATE, msg);
        }
    }
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

namespace {

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

size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

} // namespace

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
    if ((rc = ensure_bytes(c, (void **)&c->d_pack, &c->pack_bytes, (op_at + px) * sizeof(float)))) return rc;
    float *d_rgb = c->d_pack, *d_opacity = alpha_mode == NERF_ALPHA_OPAQUE ? nullptr : c->d_pack + op_at;
    if ((rc = render_device(c, cam, o, d_rgb, nullptr, d_opacity, st, stats, bg))) return rc;
    HIP_TRY(c, launch_pack_rgba8(d_rgb, d_opacity, (uint32_t *)d_rgba, px, alpha_mode, st));
    if (stats) HIP_TRY(c, hipStreamSynchronize(st)); // as the float variant: with stats the output is complete on return
    return NERF_OK;
}

// ================================================================================================
// extern "C"
// ================================================================================================
// No C++ exception may cross the C ABI (a Rust caller would abort): every entry point that can allocate is a function-try-block.
#define NERF_CATCH(c)                                                                                              \
    catch (const std::bad_alloc &) { return fail((c), NERF_ERR_IO, "out of host memory"); }                         \
    catch (const std::exception &e) { return fail((c), NERF_ERR_INVALID, std::string("internal error: ") + e.what()); } \
    catch (...) { return fail((c), NERF_ERR_INVALID, "internal error"); }

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
    if (const char *env = getenv("NERF_MAX_RAYS_PER_PASS")) {
        const long long v = atoll(env);
        if (v > 0) c->max_rays_per_pass = (size_t)v;
    }
    if (const char *env = getenv("NERF_MAX_EXPORT_BYTES")) {
        const long long v = atoll(env);
        if (v > 0) c->max_export_bytes = (size_t)v;
    }
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
    if (const char *env = getenv("NERF_GRADIENT_CHUNK")) {
        const long long v = atoll(env);
        if (v > 0) c->gradient_chunk = (size_t)v;
    }
    if (const char *env = getenv("NERF_DEBUG_NORMALS")) c->debug_normals = atoi(env) > 0;
    if (const char *env = getenv("NERF_ZERO_STEP_SKIP")) c->zero_step_skip = atoi(env) != 0;
    if (const char *env = getenv("NERF_RAY_GROUPING")) c->ray_grouping = atoi(env) != 0;
    if (const char *env = getenv("NERF_DEBUG_ZSKIP")) {
        if (atoi(env) > 0 && hipMalloc((void **)&c->d_zskip, 2 * sizeof(unsigned long long)) != hipSuccess) c->d_zskip = nullptr;
    }
    if (const char *env = getenv("NERF_DEBUG_CLOCK")) {
        if (atoi(env) > 0 && hipMalloc((void **)&c->d_clock, (size_t)c->n_cus * 2 * sizeof(unsigned long long)) != hipSuccess) c->d_clock = nullptr;
    }
    if (hipMalloc((void **)&c->d_skip, sizeof(unsigned long long)) != hipSuccess) c->d_skip = nullptr;
    if (hipMalloc((void **)&c->d_nonfinite, sizeof(unsigned int)) != hipSuccess) c->d_nonfinite = nullptr;
    // kernel attributes (dynamic LDS sizes) are per device, not per context: set them once per device and process
    static std::mutex init_mu;
    static std::set<int> init_done;
    hipError_t e1 = hipSuccess, e2 = hipSuccess;
    {
        std::lock_guard<std::mutex> lk(init_mu);
        if (!init_done.count(device_id)) {
            e1 = nerf_mlp_init();
            if (e1 == hipSuccess) e1 = nerf_mlp_bf16v2_init();
            if (e1 == hipSuccess) e1 = nerf_prefilter_f16v2_init();
#if NERF_BF16_V3
            if (e1 == hipSuccess) e1 = nerf_mlp_bf16v3_init();
#endif
            if (e1 == hipSuccess) e1 = nerf_mlp_bf16x3_init();
            if (e1 == hipSuccess) e1 = nerf_seq_init();
            if (e1 == hipSuccess) e1 = nerf_seq_bf16_init();
            if (e1 == hipSuccess) e1 = nerf_seq_x3_init();
            if (e1 == hipSuccess) e1 = nerf_mlp_f16x2_init();
            if (e1 == hipSuccess) e1 = nerf_seq_f16x2_init();
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
    for (auto &n : c->net) { if (n.wstream) (void)hipFree(n.wstream); if (n.small) (void)hipFree(n.small); if (n.small_f32) (void)hipFree(n.small_f32); if (n.wstream_bf16v2) (void)hipFree(n.wstream_bf16v2); if (n.wstream_bf16v3) (void)hipFree(n.wstream_bf16v3); if (n.wstream_x3) (void)hipFree(n.wstream_x3); if (n.wstream_x2) (void)hipFree(n.wstream_x2); if (n.wstream_f16v2) (void)hipFree(n.wstream_f16v2); }
    float *ptrs[] = {c->d_dirs, c->d_tc, c->d_sc, c->d_rgbc, c->d_tf, c->d_sf, c->d_rgbf, c->d_rayfb, c->d_rayaux, c->d_out, c->d_pack};
    for (float *p : ptrs) if (p) (void)hipFree(p);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->d_mesh) (void)hipFree(c->d_mesh);
    if (c->d_batch) (void)hipFree(c->d_batch);
    if (c->d_comp) (void)hipFree(c->d_comp);
    if (c->d_normal) (void)hipFree(c->d_normal);
    if (c->d_stencil) (void)hipFree(c->d_stencil);
    if (c->d_clock) (void)hipFree(c->d_clock);
    if (c->d_zskip) (void)hipFree(c->d_zskip);
    if (c->d_skip) (void)hipFree(c->d_skip);
    if (c->d_nonfinite) (void)hipFree(c->d_nonfinite);
    if (c->d_seq) (void)hipFree(c->d_seq);
    if (c->d_h8) (void)hipFree(c->d_h8);
    if (c->d_slot_point) (void)hipFree(c->d_slot_point);
    if (c->d_flag_list) (void)hipFree(c->d_flag_list);
    if (c->d_point_list) (void)hipFree(c->d_point_list);
    if (c->d_jstar) (void)hipFree(c->d_jstar);
    if (c->d_cert_aux) (void)hipFree(c->d_cert_aux);
    if (c->d_cert) (void)hipFree(c->d_cert);
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

int nerf_load_network_dir(nerf_ctx *c, int which, const char *dir) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!dir) return fail(c, NERF_ERR_INVALID, "dir is NULL");
    DeviceGuard dg(c->device);
    std::map<std::string, Tensor> params;
    std::string err;
    int rc = read_tensor_dir(dir, params, err);
    if (rc) return fail(c, rc, err);
    HostNet hn;
    rc = assemble_net(params, hn, err);
    if (rc) return fail(c, rc, err);
    return upload_net(c, which, hn);
} NERF_CATCH(c)

int nerf_load_network_tensors(nerf_ctx *c, int which, int n, const char *const *names, const int64_t *dims,
                              const float *const *data) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (n < 0 || (n > 0 && (!names || !dims || !data))) return fail(c, NERF_ERR_INVALID, "bad tensor table");
    DeviceGuard dg(c->device);
    std::map<std::string, Tensor> params;
    for (int i = 0; i < n; ++i) {
        if (!names[i] || !data[i] || dims[2 * i] < 0 || dims[2 * i + 1] < 0) return fail(c, NERF_ERR_INVALID, "bad tensor table entry");
        Tensor t;
        size_t cnt = (size_t)dims[2 * i];
        t.dims.push_back(dims[2 * i]);
        if (dims[2 * i + 1] > 0) { t.dims.push_back(dims[2 * i + 1]); cnt *= (size_t)dims[2 * i + 1]; }
        t.data.assign(data[i], data[i] + cnt);
        params[names[i]] = std::move(t);
    }
    HostNet hn;
    std::string err;
    const int rc = assemble_net(params, hn, err);
    if (rc) return fail(c, rc, err);
    return upload_net(c, which, hn);
} NERF_CATCH(c)

int nerf_load_network_blob(nerf_ctx *c, int which, const char *blob_path) try {
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!blob_path) return fail(c, NERF_ERR_INVALID, "blob_path is NULL");
    DeviceGuard dg(c->device);
    std::vector<float> ws, sm;
    std::string err;
    const int rrc = read_blob_file(blob_path, ws, sm, err);
    if (rrc) return fail(c, rrc, err);
    const int rc = upload_packed(c, which, ws, sm);
    return rc ? rc : bf16_from_f32_stream(c, which, ws);
} NERF_CATCH(c)

static int forward_device(nerf_ctx *c, int which, int dtype, const float *d_pts, const float *d_dirs, size_t n, float *d_rgb,
                          float *d_sigma, void *stream);

int nerf_forward_batch_device(nerf_ctx *c, int which, const float *d_pts, const float *d_dirs, size_t n, float *d_rgb,
                              float *d_sigma, void *stream) try {
    return forward_device(c, which, NERF_MLP_F32, d_pts, d_dirs, n, d_rgb, d_sigma, stream);
} NERF_CATCH(c)

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
    a.nonfinite = split_dtype(dtype) ? c->d_nonfinite : nullptr;
    HIP_TRY(c, launch_mlp(c, dtype, a, true, (hipStream_t)stream));
    return NERF_OK;
}

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
static int density_batch_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float *d_sigma, hipStream_t st) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (!d_pts || !d_sigma) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    DeviceGuard dg(c->device);
    MlpArgs a{};
    a.mode = MLP_MODE_POINTS;
    a.wstream = c->net[which].wstream; a.small_params = c->net[which].small_f32; zskip_of(c, c->net[which], a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.sigma_out = d_sigma;
    HIP_TRY(c, nerf_mlp_launch(a, false, c->n_cus, st));
    return NERF_OK;
}

int nerf_density_batch_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float *d_sigma, void *stream) try {
    return density_batch_device(c, which, d_pts, n, d_sigma, (hipStream_t)stream);
} NERF_CATCH(c)

int nerf_density_batch(nerf_ctx *c, int which, const float *pts, size_t n, float *sigma) try {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (!pts || !sigma) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    DeviceGuard dg(c->device);
    int rc;
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
    const size_t px = w * h, bytes = px * 3 * sizeof(float);
    const size_t maps = (depth_out ? 1 : 0) + (opacity_out ? 1 : 0);
    if ((rc = ensure_bytes(c, (void **)&c->d_out, &c->out_floats, bytes + maps * px * sizeof(float)))) return rc;
    float *d_depth = depth_out ? c->d_out + 3 * px : nullptr;
    float *d_opacity = opacity_out ? c->d_out + (3 + (depth_out ? 1 : 0)) * px : nullptr;
    nerf_stats local; // a synchronous render always reads its counters: a frame computed outside a split arithmetic's range is an error
    if ((rc = render_device(c, cam, opts, c->d_out, d_depth, d_opacity, c->stream, stats ? stats : &local))) return rc;
    HIP_TRY(c, hipMemcpyAsync(rgb_out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    if (d_depth) HIP_TRY(c, hipMemcpyAsync(depth_out, d_depth, px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (d_opacity) HIP_TRY(c, hipMemcpyAsync(opacity_out, d_opacity, px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
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
    const size_t bytes = w * h * 4; // 4 bytes per pixel come back instead of 12 (16 with the opacity)
    if ((rc = ensure_bytes(c, (void **)&c->d_out, &c->out_floats, bytes))) return rc;
    nerf_stats local; // a synchronous render always reads its counters (see nerf_render_image_aux)
    if ((rc = render_rgba8_device(c, cam, opts, background, alpha_mode, (uint8_t *)c->d_out, c->stream, stats ? stats : &local))) return rc;
    HIP_TRY(c, hipMemcpyAsync(rgba_out, c->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
} NERF_CATCH(c)

// ---- ray batches ---------------------------------------------------------------------------------------------------------------------
// nerf_render_rays_device and nerf_render_rays_normals_device (want_normals)
static int rays_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_,
                       float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts, const float background[3],
                       float *d_rgb_out, float *d_depth_out, float *d_opacity_out, bool want_normals, float h, float *d_normals_out, void *stream,
                       nerf_stats *stats) {
    int rc;
    if ((rc = check_ray_batch(c, d_origins, n_origins, d_dirs, n_rays, near_, far_, d_bounds, opts, background, d_rgb_out))) return rc;
    if (want_normals && (rc = check_normals(c, h, d_normals_out))) return rc;
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    const hipStream_t st = (hipStream_t)stream;
    RayBatch b{nullptr, nullptr, d_dirs, n_rays, normalize ? 1 : 0, near_, far_, d_bounds, d_rng_index};
    float origin[3];
    if (n_origins == 1) { // the shared origin rides in the MLP kernels' arguments: 12 bytes come back first
        HIP_TRY(c, hipMemcpyAsync(origin, d_origins, sizeof origin, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        b.h_origin = origin;
    } else b.d_origins = d_origins;
    return render_rays_device(c, b, opts, background, d_rgb_out, d_depth_out, d_opacity_out, st, stats, h, want_normals ? d_normals_out : nullptr);
}

int nerf_render_rays_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize, float near_,
                            float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts, const float background[3],
                            float *d_rgb_out, float *d_depth_out, float *d_opacity_out, void *stream, nerf_stats *stats) try {
    return rays_device(c, d_origins, n_origins, d_dirs, n_rays, normalize, near_, far_, d_bounds, d_rng_index, opts, background, d_rgb_out, d_depth_out,
                       d_opacity_out, false, 0.0f, nullptr, stream, stats);
} NERF_CATCH(c)

int nerf_render_rays_normals_device(nerf_ctx *c, const float *d_origins, size_t n_origins, const float *d_dirs, size_t n_rays, int normalize,
                                    float near_, float far_, const float *d_bounds, const uint32_t *d_rng_index, const nerf_render_opts *opts,
                                    const float background[3], float *d_rgb_out, float *d_depth_out, float *d_opacity_out, float h,
                                    float *d_normals_out, void *stream, nerf_stats *stats) try {
    return rays_device(c, d_origins, n_origins, d_dirs, n_rays, normalize, near_, far_, d_bounds, d_rng_index, opts, background, d_rgb_out, d_depth_out,
                       d_opacity_out, true, h, d_normals_out, stream, stats);
} NERF_CATCH(c)

// nerf_render_rays and nerf_render_rays_normals (want_normals)
static int rays_host(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_,
                     const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3], float *rgb_out,
                     float *depth_out, float *opacity_out, bool want_normals, float h, float *normals_out, nerf_stats *stats) {
    int rc;
    if ((rc = check_ray_batch(c, origins, n_origins, dirs, n_rays, near_, far_, bounds, opts, background, rgb_out))) return rc;
    if (want_normals && (rc = check_normals(c, h, normals_out))) return rc;
    if ((rc = check_ray_batch_rays(c, origins, n_origins, dirs, n_rays, normalize, bounds))) return rc;
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n_rays == 0) return NERF_OK;
    DeviceGuard dg(c->device);
    // staging (floats): dirs, [origins], [bounds], [rng_index], rgb, [depth], [opacity], [normals]
    const size_t R = n_rays, o_d = 0, o_o = o_d + 3 * R, o_b = o_o + (n_origins == 1 ? 0 : 3 * R), o_i = o_b + (bounds ? 2 * R : 0),
                 o_c = o_i + (rng_index ? R : 0), o_z = o_c + 3 * R, o_a = o_z + (depth_out ? R : 0), o_n = o_a + (opacity_out ? R : 0),
                 total = o_n + (want_normals ? 3 * R : 0);
    if ((rc = ensure_bytes(c, (void **)&c->d_out, &c->out_floats, total * sizeof(float)))) return rc;
    float *d = c->d_out;
    HIP_TRY(c, hipMemcpyAsync(d + o_d, dirs, 3 * R * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (n_origins != 1) HIP_TRY(c, hipMemcpyAsync(d + o_o, origins, 3 * R * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (bounds) HIP_TRY(c, hipMemcpyAsync(d + o_b, bounds, 2 * R * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (rng_index) HIP_TRY(c, hipMemcpyAsync(d + o_i, rng_index, R * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    RayBatch b{n_origins == 1 ? origins : nullptr, n_origins == 1 ? nullptr : d + o_o, d + o_d, n_rays, normalize ? 1 : 0, near_, far_,
               bounds ? d + o_b : nullptr, rng_index ? (const uint32_t *)(d + o_i) : nullptr};
    nerf_stats local; // a synchronous render always reads its counters (see nerf_render_image_aux)
    if ((rc = render_rays_device(c, b, opts, background, d + o_c, depth_out ? d + o_z : nullptr, opacity_out ? d + o_a : nullptr, c->stream,
                                 stats ? stats : &local, h, want_normals ? d + o_n : nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(rgb_out, d + o_c, 3 * R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (want_normals) HIP_TRY(c, hipMemcpyAsync(normals_out, d + o_n, 3 * R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (depth_out) HIP_TRY(c, hipMemcpyAsync(depth_out, d + o_z, R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (opacity_out) HIP_TRY(c, hipMemcpyAsync(opacity_out, d + o_a, R * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
}

int nerf_render_rays(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_,
                     const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3], float *rgb_out,
                     float *depth_out, float *opacity_out, nerf_stats *stats) try {
    return rays_host(c, origins, n_origins, dirs, n_rays, normalize, near_, far_, bounds, rng_index, opts, background, rgb_out, depth_out, opacity_out,
                     false, 0.0f, nullptr, stats);
} NERF_CATCH(c)

int nerf_render_rays_normals(nerf_ctx *c, const float *origins, size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_,
                             float far_, const float *bounds, const uint32_t *rng_index, const nerf_render_opts *opts, const float background[3],
                             float *rgb_out, float *depth_out, float *opacity_out, float h, float *normals_out, nerf_stats *stats) try {
    return rays_host(c, origins, n_origins, dirs, n_rays, normalize, near_, far_, bounds, rng_index, opts, background, rgb_out, depth_out, opacity_out,
                     true, h, normals_out, stats);
} NERF_CATCH(c)

// ---- density gradients at caller points (normal_kernels.hip around the sigma-only launch) -----------------------------------------------
// The points run in chunks of at most c->gradient_chunk (and of what one MLP launch takes for six stencil points each): per chunk
// stencil -> sigma-only MLP over 6 m points -> combine, all on `st`, nothing comes back to the host.  A point's gradient depends on that
// point alone (the sigma-only kernel's bits do not depend on the slot), so the chunking shows in no bit.
static int density_gradient_device(nerf_ctx *c, int which, const float *d_pts, size_t n, float h, float *d_grad, hipStream_t st) {
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!(std::isfinite(h) && h > 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and greater than 0");
    if (n > 0 && (!d_pts || !d_grad)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    DeviceGuard dg(c->device);
    const size_t chunk = std::max<size_t>(1, std::min({c->gradient_chunk, n, max_batch_points(c->n_cus) / 6}));
    int rc;
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
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail(c, NERF_ERR_INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE");
    if (!(std::isfinite(h) && h > 0.0f)) return fail(c, NERF_ERR_INVALID, "h (the central-difference step) must be finite and greater than 0");
    if (n > 0 && (!pts || !grad)) return fail(c, NERF_ERR_INVALID, "NULL buffer");
    if (!c) return fail(nullptr, NERF_ERR_INVALID, "ctx is NULL");
    if (n == 0) return NERF_OK;
    if (n > max_batch_points(c->n_cus)) return fail(c, NERF_ERR_INVALID, "batch too large (n plus one grid stride of tiles must fit in int32)");
    if (!c->net[which].loaded) return fail(c, NERF_ERR_STATE, "network not loaded");
    DeviceGuard dg(c->device);
    int rc;
    if ((rc = ensure_bytes(c, &c->d_scratch, &c->scratch_bytes, n * 6 * sizeof(float)))) return rc;
    float *d_pts = (float *)c->d_scratch, *d_grad = d_pts + 3 * n;
    HIP_TRY(c, hipMemcpyAsync(d_pts, pts, 3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = density_gradient_device(c, which, d_pts, n, h, d_grad, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(grad, d_grad, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NERF_OK;
} NERF_CATCH(c)

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
        // last_render may still list these pairs (kind 1); it never recycles them, and they are not read again
        for (auto &p : c->last_render) if (p.kind == 1) p.kind = 3;
        c->last_render.erase(std::remove_if(c->last_render.begin(), c->last_render.end(), [](const EvPair &p) { return p.kind == 3; }), c->last_render.end());
        recycle_dominant(c, 0);
    }
    return NERF_OK;
} NERF_CATCH(c)

int nerf_debug_shader_clock_mhz(nerf_ctx *c, double *mhz) try {
    if (!c || !mhz) return fail(c, NERF_ERR_INVALID, "NULL argument");
    if (!c->d_clock || !c->clock_valid) return fail(c, NERF_ERR_STATE, "set NERF_DEBUG_CLOCK=1 before nerf_create and render a frame first");
    DeviceGuard dg(c->device);
    std::vector<unsigned long long> h((size_t)c->n_cus * 2);
    HIP_TRY(c, hipDeviceSynchronize());
    HIP_TRY(c, hipMemcpy(h.data(), c->d_clock, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> f;
    for (int i = 0; i < c->n_cus; ++i) if (h[2 * i + 1] > 0) f.push_back(100.0 * (double)h[2 * i] / (double)h[2 * i + 1]);
    if (f.empty()) return fail(c, NERF_ERR_STATE, "no clock samples");
    std::sort(f.begin(), f.end());
    *mhz = f[f.size() / 2];
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
                          float *t_new_out, float *t_fine_out, float tau, uint8_t *flags_out);

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

} // extern "C"
