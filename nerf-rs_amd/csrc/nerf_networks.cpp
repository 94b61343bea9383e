// nerf_networks.cpp -- the networks on the device: upload of a loaded network in every arithmetic's weight stream (the 16-bit streams are
// re-packed here from one piece order), which stream and which kernel a dtype selects, and the nerf_load_network_* entry points.
#include <hip/hip_runtime.h>

#include <map>

#include "../../include/nerf_mi355x.h"
#include "host_util.h"
#include "mlp_kernel.h"
#include "mlp_layout.h"

using namespace nerfhost;

#include "nerf_internal.h"

using namespace nerfint;

namespace nerfint {

const float *stream_of(const DevNet &n, int dtype) {
    if (dtype == NERF_MLP_BF16X3) return (const float *)n.wstream_x3;
    if (dtype == NERF_MLP_F16X2) return (const float *)n.wstream_x2;
    if (dtype == NERF_MLP_F32) return n.wstream;
    return (const float *)n.wstream_bf16v2;
}
const float *small_of(const DevNet &n, int dtype) { return dtype == NERF_MLP_F32 ? n.small_f32 : n.small; }
// zero-step skipping of the f32 kernels (MlpArgs / SeqArgs; the other arithmetics ignore the two fields): per network, decided at load
// ... and the context's ray grouping and wave tiling (MlpArgs.ray_grouping, .wave_tiling: the ray-mode launcher of the f32 kernels reads
// them, nothing else does; tiling also needs MlpArgs.rays_per_row, which only an image pass knows: nerf_render.cpp eval_net)
void zskip_of(const nerf_ctx *c, const DevNet &n, MlpArgs &a) {
    a.zero_skip = n.zero_skip ? 1 : 0; a.zskip_stats = c->d_zskip;
    a.ray_grouping = c->ray_grouping ? 1 : 0; a.wave_tiling = c->wave_tiling ? 1 : 0;
    a.depth_order = c->depth_order ? 1 : 0; a.tile_rotation = c->tile_rotation ? 1 : 0; // the table itself is the pass pipeline's (nerf_render.cpp eval_net)
}
void zskip_of(const nerf_ctx *c, const DevNet &n, SeqArgs &a) { a.zero_skip = n.zero_skip ? 1 : 0; a.zskip_stats = c->d_zskip; }

hipError_t init_mlp_kernels() {
    hipError_t e1 = nerf_mlp_init();
    if (e1 == hipSuccess) e1 = nerf_mlp_bf16v2_init();
    if (e1 == hipSuccess) e1 = nerf_prefilter_f16v2_init();
    if (e1 == hipSuccess) e1 = nerf_mlp_bf16x3_init();
    if (e1 == hipSuccess) e1 = nerf_seq_init();
    if (e1 == hipSuccess) e1 = nerf_seq_bf16_init();
    if (e1 == hipSuccess) e1 = nerf_seq_x3_init();
    if (e1 == hipSuccess) e1 = nerf_mlp_f16x2_init();
    if (e1 == hipSuccess) e1 = nerf_seq_f16x2_init();
    return e1;
}

hipError_t launch_mlp(const nerf_ctx *c, int dtype, const MlpArgs &a, bool full, hipStream_t st) {
    if (dtype == NERF_MLP_F32) return nerf_mlp_launch(a, full, c->n_cus, st);
    if (dtype == NERF_MLP_BF16X3) return nerf_mlp_bf16x3_launch(a, full, c->n_cus, st);
    if (dtype == NERF_MLP_F16X2) return nerf_mlp_f16x2_launch(a, full, c->n_cus, st);
    return nerf_mlp_bf16v2_launch(a, full, c->n_cus, st);
}

hipError_t launch_sigma_points(const nerf_ctx *c, const DevNet &net, const float *d_pts, size_t n, float *d_sigma, hipStream_t st) {
    MlpArgs a{};
    a.mode = MLP_MODE_POINTS;
    a.wstream = net.wstream; a.small_params = net.small_f32; zskip_of(c, net, a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.sigma_out = d_sigma;
    return launch_mlp(c, NERF_MLP_F32, a, false, st);
}

} // namespace nerfint

namespace {

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
        c->cert_prefilter_f16[which] = c->cert_allow_f16 && d.wstream_f16v2 != nullptr;
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

} // namespace

extern "C" {

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

} // extern "C"
