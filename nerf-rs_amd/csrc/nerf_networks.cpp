// nerf_networks.cpp -- the networks on the device: the table that says which stream and which kernels an arithmetic selects, the upload of a
// loaded network in every arithmetic's weight stream, and the nerf_load_network_* entry points.
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

const Arith &arith_of(int dtype) {
    static const Arith table[] = { // indexed by NERF_MLP_*
        {NET_F32, NET_SMALL_F32, {nerf_mlp_init, nerf_seq_init}, nerf_mlp_launch, nerf_trunk_seq_launch, nullptr, 0, nullptr, false},
        {NET_BF16V2, NET_SMALL, {nerf_mlp_bf16v2_init, nerf_seq_bf16_init}, nerf_mlp_bf16v2_launch, nerf_trunk_seq_bf16_launch, nerf_colour_bf16_launch,
         512, nerf_seq_h8_bytes_bf16, false},
        {NET_X3, NET_SMALL, {nerf_mlp_bf16x3_init, nerf_seq_x3_init}, nerf_mlp_bf16x3_launch, nerf_trunk_seq_x3_launch, nerf_colour_x3_launch,
         1024, nerf_seq_h8_bytes, true},
        {NET_X2, NET_SMALL, {nerf_mlp_f16x2_init, nerf_seq_f16x2_init}, nerf_mlp_f16x2_launch, nerf_trunk_seq_f16x2_launch, nerf_colour_f16x2_launch,
         1024, nerf_seq_h8_bytes, true},
    };
    static_assert(NERF_MLP_F32 == 0 && NERF_MLP_BF16 == 1 && NERF_MLP_BF16X3 == 2 && NERF_MLP_F16X2 == 3, "the table's order");
    return table[dtype];
}

const Prefilter &prefilter_of(bool f16) {
    static const Prefilter table[] = { // the f16 twin's launchers exist sigma-only, without export: they take no such switch
        {NET_BF16V2, nullptr, nerf_mlp_bf16v2_launch, nerf_trunk_seq_bf16_launch, false},
        {NET_F16V2, nerf_prefilter_f16v2_init,
         [](const MlpArgs &a, bool, int n_blocks, hipStream_t st) { return nerf_mlp_f16v2_launch(a, n_blocks, st); },
         [](const SeqArgs &a, bool, int n_blocks, hipStream_t st) { return nerf_trunk_seq_f16v2_launch(a, n_blocks, st); }, true},
    };
    return table[f16 ? 1 : 0];
}

void fill_net(const nerf_ctx *c, const DevNet &n, int dtype, MlpArgs &a) {
    const Arith &ar = arith_of(dtype);
    a.wstream = n.at(ar.stream); a.small_params = n.at(ar.small);
    a.zero_skip = n.zero_skip ? 1 : 0; a.zskip_stats = c->dev<unsigned long long>(BUF_ZSKIP);
    a.ray_grouping = c->ray_grouping ? 1 : 0; a.wave_tiling = c->wave_tiling ? 1 : 0;
    a.depth_order = c->depth_order ? 1 : 0; a.tile_rotation = c->tile_rotation ? 1 : 0; // the table itself is the pass pipeline's (nerf_render.cpp eval_net)
    a.nonfinite = ar.counts_range ? c->dev<unsigned int>(BUF_NONFINITE) : nullptr;
}
void fill_net(const nerf_ctx *c, const DevNet &n, int dtype, SeqArgs &a) {
    const Arith &ar = arith_of(dtype);
    a.wstream = n.at(ar.stream); a.small_params = n.at(ar.small);
    a.zero_skip = n.zero_skip ? 1 : 0; a.zskip_stats = c->dev<unsigned long long>(BUF_ZSKIP);
    a.nonfinite = ar.counts_range ? c->dev<unsigned int>(BUF_NONFINITE) : nullptr;
}

hipError_t init_mlp_kernels() {
    hipError_t e = hipSuccess;
    for (int dt = NERF_MLP_F32; dt <= NERF_MLP_F16X2 && e == hipSuccess; ++dt)
        for (auto init : arith_of(dt).init) if (e == hipSuccess) e = init();
    for (int f16 = 0; f16 < 2 && e == hipSuccess; ++f16) if (prefilter_of(f16).init) e = prefilter_of(f16).init();
    return e;
}

hipError_t launch_sigma_points(const nerf_ctx *c, const DevNet &net, const float *d_pts, size_t n, float *d_sigma, hipStream_t st) {
    MlpArgs a{};
    a.mode = MLP_MODE_POINTS;
    fill_net(c, net, NERF_MLP_F32, a);
    a.n_points = (int)n; a.pts_soa = d_pts; a.sigma_out = d_sigma;
    return launch_mlp(c, NERF_MLP_F32, a, false, st);
}

} // namespace nerfint

namespace {

template <class T>
int upload(nerf_ctx *c, DevBuf &b, const std::vector<T> &v) { // an empty vector releases the buffer: that stream is unavailable
    if (v.empty()) return b.release(c);
    const int rc = b.ensure(c, v.size() * sizeof(T));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return NERF_OK;
}

// One network, from its packed f32 image (a directory's or tensor table's pack_network, or a blob), in every arithmetic's form.
int upload_network(nerf_ctx *c, int which, const std::vector<float> &ws, const std::vector<float> &sm) {
    if (ws.size() != (size_t)nerfmlp::kChunksFull * nerfmlp::kChunkFloats || sm.size() != (size_t)nerfmlp::kSmallFloats)
        return fail(c, NERF_ERR_SHAPE, "packed network image has the wrong size for this library build");
    // the f32 kernels run the bottleneck folded into viewdirs (once per loaded network); the 16-bit arithmetics keep the packed image's small block
    std::vector<float> fws, fsm;
    if (!fold_network(ws, sm, fws, fsm)) return fail(c, NERF_ERR_SHAPE, "internal: folded network image has the wrong size");
    NetStreams s;
    if (!build_streams(ws, s)) return fail(c, NERF_ERR_SHAPE, "internal: 16-bit stream sizes");
    DevNet &d = c->net[which];
    d.loaded = false; // until every stream below is on the device
    int rc;
    if ((rc = upload(c, d.buf[NET_F32], fws)) || (rc = upload(c, d.buf[NET_SMALL], sm)) || (rc = upload(c, d.buf[NET_SMALL_F32], fsm)) ||
        (rc = upload(c, d.buf[NET_BF16V2], s.bf16v2)) || (rc = upload(c, d.buf[NET_X3], s.x3)) || (rc = upload(c, d.buf[NET_F16V2], s.f16v2)) ||
        (rc = upload(c, d.buf[NET_X2], s.x2))) return rc;
    d.zero_skip = c->zero_step_skip && zero_skip_safe(fws, fsm); // exact only while every parameter is finite (mlp_f32_core.hip.h tile_steps)
    // certify_zero calibrates itself per network: margins start at the floors of the pre-filter this network gets (f16 where its weights fit)
    c->cert_prefilter_f16[which] = c->cert_allow_f16 && d.buf[NET_F16V2].p != nullptr;
    c->cert_margin[which] = c->cert_prefilter_f16[which] ? c->cert_margin_floor_f16[which] : c->cert_margin_floor[which];
    d.loaded = true;
    return NERF_OK;
}

int upload_net(nerf_ctx *c, int which, const HostNet &hn) {
    std::vector<float> ws, sm;
    pack_network(hn, ws, sm);
    return upload_network(c, which, ws, sm);
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
    return upload_network(c, which, ws, sm);
} NERF_CATCH(c)

} // extern "C"
