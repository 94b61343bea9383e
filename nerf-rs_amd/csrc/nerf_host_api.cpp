// nerf_host_api.cpp -- the HOST-ONLY entry points of the C ABI (include/nerf_mi355x.h): everything that parses files from disk or
// converts host buffers and never touches the device -- weight-directory validation and packing, the packed-blob reader, camera
// construction (incl. the hand-written JSON reader), PPM / PFM / PAM / PLY writers, quantisers, the split diagnostics, the ray-clip walk on the CPU (ray_clip_core.h).  No HIP header is included,
// so this file and host_util.cpp also build with plain g++ under AddressSanitizer + UBSan (`make host-asan`; driven by
// tests/test_host_asan.py on the CPU box with truncated / oversized / malformed inputs).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"
#include "host_util.h"
#include "mlp_layout.h"
#include "ray_clip_core.h"

using namespace nerfhost;

namespace nerfhost {

static thread_local std::string g_err; // message of the last failing context-free call on this thread

int fail_noctx(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

const char *last_error_noctx() { return g_err.c_str(); }

static const char kBlobMagic[8] = {'N', 'R', 'F', 'M', 'I', '3', '5', '5'};

// Blob layout (include/nerf_mi355x.h): 16-byte header {"NRFMI355", u32 version = 1, u32 n_floats} + weight stream + small block.
// The sizes are fixed by this build's layout; anything else -- short file, trailing bytes, other version -- is refused.
int read_blob_file(const std::string &path, std::vector<float> &ws, std::vector<float> &sm, std::string &err) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { err = "read blob: " + path; return NERF_ERR_IO; }
    char magic[8]; uint32_t hdr[2] = {0, 0};
    const size_t nw = (size_t)nerfmlp::kChunksFull * nerfmlp::kChunkFloats, ns = nerfmlp::kSmallFloats;
    ws.assign(nw, 0.f); sm.assign(ns, 0.f);
    const bool ok = fread(magic, 1, 8, f) == 8 && fread(hdr, 4, 2, f) == 2 && !memcmp(magic, kBlobMagic, 8) && hdr[0] == 1u &&
                    hdr[1] == nw + ns && fread(ws.data(), 4, nw, f) == nw && fread(sm.data(), 4, ns, f) == ns && fgetc(f) == EOF;
    fclose(f);
    if (!ok) { err = "not a version-1 packed network blob for this build: " + path; return NERF_ERR_SHAPE; }
    return NERF_OK;
}

} // namespace nerfhost

// No C++ exception may cross the C ABI (a Rust caller would abort).
#define NERF_HOST_CATCH                                                                                             \
    catch (const std::bad_alloc &) { return fail_noctx(NERF_ERR_IO, "out of host memory"); }                        \
    catch (const std::exception &e) { return fail_noctx(NERF_ERR_INVALID, std::string("internal error: ") + e.what()); } \
    catch (...) { return fail_noctx(NERF_ERR_INVALID, "internal error"); }

#ifndef NERF_BUILD_VARIANT
#define NERF_BUILD_VARIANT ""
#endif

extern "C" {

const char *nerf_build_variant(void) { return NERF_BUILD_VARIANT; }

int nerf_pack_network_dir(const char *dir, const char *blob_path) try {
    if (!dir || !blob_path) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::map<std::string, Tensor> params;
    std::string err;
    int rc = read_tensor_dir(dir, params, err);
    if (rc) return fail_noctx(rc, err);
    HostNet hn;
    rc = assemble_net(params, hn, err);
    if (rc) return fail_noctx(rc, err);
    std::vector<float> ws, sm;
    pack_network(hn, ws, sm);
    FILE *f = fopen(blob_path, "wb");
    if (!f) return fail_noctx(NERF_ERR_IO, std::string("cannot create ") + blob_path);
    const uint32_t hdr[2] = {1u, (uint32_t)(ws.size() + sm.size())};
    const bool ok = fwrite(kBlobMagic, 1, 8, f) == 8 && fwrite(hdr, 4, 2, f) == 2 &&
                    fwrite(ws.data(), 4, ws.size(), f) == ws.size() && fwrite(sm.data(), 4, sm.size(), f) == sm.size();
    fclose(f);
    return ok ? NERF_OK : fail_noctx(NERF_ERR_IO, std::string("short write ") + blob_path);
} NERF_HOST_CATCH

int nerf_camera_from_pose(const float c2w[12], float ref_h, float ref_w, float focal, float near_, float far_, int width,
                          int height, nerf_camera *out) try {
    if (!c2w || !out) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    const float origin[3] = {c2w[3], c2w[7], c2w[11]};
    const float forward[3] = {-c2w[2], -c2w[6], -c2w[10]};
    const float up[3] = {c2w[1], c2w[5], c2w[9]};
    const float hwf[3] = {ref_h, ref_w, focal};
    camera_from_values(near_, far_, origin, forward, up, hwf, width, height, out);
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_check_network_dir(const char *dir) try {
    if (!dir) return fail_noctx(NERF_ERR_INVALID, "dir is NULL");
    std::map<std::string, Tensor> params;
    std::string err;
    int rc = read_tensor_dir(dir, params, err);
    if (rc) return fail_noctx(rc, err);
    HostNet hn;
    rc = assemble_net(params, hn, err);
    if (rc) return fail_noctx(rc, err);
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_split_bf16x3(const float *values, size_t n, uint16_t *parts) try {
    if ((!values || !parts) && n) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < n; ++i) split_bf16x3(values[i], parts + 3 * i);
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_certify_policy(float margin, uint64_t audited, uint64_t violations, float headroom, float max_error, float *new_margin) {
    if (!(margin > 0.0f)) return fail_noctx(NERF_ERR_INVALID, "margin must be > 0");
    return certify_policy(margin, audited, violations, headroom, max_error, new_margin);
}

int nerf_debug_split_f16x2(const float *values, size_t n, uint16_t *parts) try {
    if ((!values || !parts) && n) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    for (size_t i = 0; i < n; ++i) split_f16x2(values[i], parts + 2 * i);
    return NERF_OK;
} NERF_HOST_CATCH

static int debug_pack(const char *dir, bool folded, float *wstream, size_t wstream_cap, float *small, size_t small_cap,
                      size_t *wstream_len, size_t *small_len) {
    if (!dir) return fail_noctx(NERF_ERR_INVALID, "dir is NULL");
    std::map<std::string, Tensor> params;
    std::string err;
    int rc = read_tensor_dir(dir, params, err);
    if (rc) return fail_noctx(rc, err);
    HostNet hn;
    rc = assemble_net(params, hn, err);
    if (rc) return fail_noctx(rc, err);
    std::vector<float> ws, sm;
    pack_network(hn, ws, sm);
    if (folded) {
        std::vector<float> fws, fsm;
        if (!fold_network(ws, sm, fws, fsm)) return fail_noctx(NERF_ERR_SHAPE, "internal: packed image has the wrong size");
        ws.swap(fws); sm.swap(fsm);
    }
    if (wstream_len) *wstream_len = ws.size();
    if (small_len) *small_len = sm.size();
    if (wstream) { if (wstream_cap < ws.size()) return fail_noctx(NERF_ERR_INVALID, "wstream buffer too small"); memcpy(wstream, ws.data(), ws.size() * sizeof(float)); }
    if (small) { if (small_cap < sm.size()) return fail_noctx(NERF_ERR_INVALID, "small buffer too small"); memcpy(small, sm.data(), sm.size() * sizeof(float)); }
    return NERF_OK;
}

int nerf_debug_pack_network_dir(const char *dir, float *wstream, size_t wstream_cap, float *small, size_t small_cap,
                                size_t *wstream_len, size_t *small_len) try {
    return debug_pack(dir, false, wstream, wstream_cap, small, small_cap, wstream_len, small_len);
} NERF_HOST_CATCH

int nerf_debug_fold_network_dir(const char *dir, float *wstream, size_t wstream_cap, float *small, size_t small_cap,
                                size_t *wstream_len, size_t *small_len) try {
    return debug_pack(dir, true, wstream, wstream_cap, small, small_cap, wstream_len, small_len);
} NERF_HOST_CATCH

int nerf_debug_network_stream_dir(const char *dir, int kind, uint16_t *out, size_t cap, size_t *n, int *available) try {
    if (kind < NERF_STREAM_BF16V2 || kind > NERF_STREAM_F16X2) return fail_noctx(NERF_ERR_INVALID, "kind must be one of NERF_STREAM_*");
    size_t nw = 0;
    int rc = debug_pack(dir, false, nullptr, 0, nullptr, 0, &nw, nullptr);
    if (rc) return rc;
    std::vector<float> ws(nw);
    if ((rc = debug_pack(dir, false, ws.data(), nw, nullptr, 0, nullptr, nullptr))) return rc;
    NetStreams s;
    if (!build_streams(ws, s)) return fail_noctx(NERF_ERR_SHAPE, "internal: packed image has the wrong size");
    const std::vector<uint16_t> *of[] = {&s.bf16v2, &s.f16v2, &s.x3, &s.x2};
    const std::vector<uint16_t> &v = *of[kind];
    if (available) *available = v.empty() ? 0 : 1;
    if (n) *n = v.size();
    if (out && !v.empty()) { if (cap < v.size()) return fail_noctx(NERF_ERR_INVALID, "stream buffer too small"); memcpy(out, v.data(), v.size() * sizeof(uint16_t)); }
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_zero_skip_network_dir(const char *dir, int *eligible) try {
    if (!eligible) return fail_noctx(NERF_ERR_INVALID, "eligible is NULL");
    size_t nw = 0, ns = 0;
    int rc = debug_pack(dir, true, nullptr, 0, nullptr, 0, &nw, &ns);
    if (rc) return rc;
    std::vector<float> ws(nw), sm(ns);
    rc = debug_pack(dir, true, ws.data(), nw, sm.data(), ns, nullptr, nullptr);
    if (rc) return rc;
    *eligible = zero_skip_safe(ws, sm) ? 1 : 0;
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_ray_grouping(int n_rays, int samples_per_ray, int enabled, int32_t *first_slot_of_wave_tile) try {
    using namespace nerfmlp;
    if (n_rays <= 0 || samples_per_ray <= 0 || !first_slot_of_wave_tile) return fail_noctx(NERF_ERR_INVALID, "n_rays and samples_per_ray must be > 0, the table not NULL");
    const long long n_points = (long long)n_rays * samples_per_ray;
    if (n_points > INT32_MAX - kPointsPerBlock) return fail_noctx(NERF_ERR_INVALID, "too many samples for one launch");
    const int n_tiles = ((int)n_points + kPointsPerBlock - 1) / kPointsPerBlock;
    const RayGrouping g = ray_grouping_of((int)n_points, samples_per_ray, enabled != 0); // as the ray-mode launcher of the f32 kernels (mlp_kernel.hip)
    for (int tile = 0; tile < n_tiles; ++tile)
        for (int wave = 0; wave < kWavesPerBlock; ++wave)
            first_slot_of_wave_tile[tile * kWavesPerBlock + wave] = ray_group_first_slot(tile, wave, g.segments, g.group_tiles);
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_wave_tiling(int rows, int rays_per_row, int samples_per_ray, int full, int ray_grouping, int wave_tiling, int32_t *slot) try {
    using namespace nerfmlp;
    if (rows <= 0 || rays_per_row <= 0 || samples_per_ray <= 0 || !slot) return fail_noctx(NERF_ERR_INVALID, "rows, rays_per_row and samples_per_ray must be > 0, the table not NULL");
    const long long n_points = (long long)rows * rays_per_row * samples_per_ray;
    if (n_points > INT32_MAX - kPointsPerBlock) return fail_noctx(NERF_ERR_INVALID, "too many samples for one launch");
    const int n = (int)n_points, n_tiles = (n + kPointsPerBlock - 1) / kPointsPerBlock;
    // as the ray-mode launcher of the f32 kernels (mlp_kernel.hip launch_mlp_rays), then lane by lane as the kernel
    const RayLaunchMap m = ray_launch_map_of(n, samples_per_ray, rays_per_row, full != 0, ray_grouping != 0, wave_tiling != 0);
    for (int tile = 0; tile < n_tiles; ++tile)
        for (int wave = 0; wave < kWavesPerBlock; ++wave)
            for (int p = 0; p < kPointsPerWave; ++p) {
                const int s = ray_launch_slot(m, tile, wave, p, m.wt.ss ? wave_tile_lane_part(m.wt, p) : p);
                slot[((size_t)tile * kWavesPerBlock + wave) * kPointsPerWave + p] = s < n ? s : -1;
            }
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_tile_rotation(int n_tiles, int n_workgroups, int rotation, int32_t *workgroup_of_tile, int32_t *round_of_tile) try {
    using namespace nerfmlp;
    if (n_tiles <= 0 || n_workgroups <= 0 || !workgroup_of_tile || !round_of_tile) return fail_noctx(NERF_ERR_INVALID, "n_tiles and n_workgroups must be > 0, the tables not NULL");
    if ((long long)n_tiles + 2ll * n_workgroups > INT32_MAX) return fail_noctx(NERF_ERR_INVALID, "too many tiles");
    for (int t = 0; t < n_tiles; ++t) workgroup_of_tile[t] = round_of_tile[t] = -1;
    // as the tile loop of the fused f32 kernel (mlp_kernel.hip): workgroup c starts at tile c and walks on with tile_walk_next while the tile
    // lies below n_tiles; a tile taken twice keeps -2
    for (int c = 0; c < n_workgroups; ++c) {
        TileWalk w = {0, 0};
        int k = 0;
        for (int tile = c; tile < n_tiles; tile = tile_walk_next(w, c, n_workgroups, rotation != 0), ++k) {
            if (rotation && tile != rotated_tile(k, c, n_workgroups)) return fail_noctx(NERF_ERR_INVALID, "internal error: the walk left rotated_tile");
            workgroup_of_tile[tile] = workgroup_of_tile[tile] == -1 ? c : -2;
            round_of_tile[tile] = k;
        }
    }
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_debug_coarse_cut_walk(int rows, int rays_per_row, int samples_per_ray, int ray_grouping, int cut_block, int cut_after, int32_t *tiles,
                               size_t tiles_cap, int32_t *blocks, int32_t *block_tiles) try {
    using namespace nerfmlp;
    if (rows <= 0 || rays_per_row <= 0 || samples_per_ray <= 0 || !tiles) return fail_noctx(NERF_ERR_INVALID, "rows, rays_per_row and samples_per_ray must be > 0, the table not NULL");
    const long long n_points = (long long)rows * rays_per_row * samples_per_ray;
    if (n_points > INT32_MAX - kPointsPerBlock) return fail_noctx(NERF_ERR_INVALID, "too many samples for one launch");
    const int n = (int)n_points, n_tiles = (n + kPointsPerBlock - 1) / kPointsPerBlock;
    if (tiles_cap < (size_t)n_tiles) return fail_noctx(NERF_ERR_INVALID, "the table holds fewer entries than the launch has tiles");
    // as the ray-mode launcher of the f32 kernels (mlp_kernel.hip launch_mlp_rays) for a sampling launch, then unit by unit as the kernel's
    // workgroups: a unit's first tile, then ray_cut_next_in_unit until it says the unit is finished
    const RayCutWalk w = ray_cut_walk_of(ray_cut_map_of(ray_launch_map_of(n, samples_per_ray, rays_per_row, false, ray_grouping != 0, true)), n);
    if (blocks) *blocks = w.blocks;
    if (block_tiles) *block_tiles = w.block_tiles;
    int visited = 0;
    if (w.blocks == 0) { // the launch does not qualify: it keeps the static walk (nerf_debug_tile_rotation), every tile in turn here
        for (int t = 0; t < n_tiles; ++t) tiles[visited++] = t;
        return visited;
    }
    for (int u = 0; u < ray_cut_units(w); ++u)
        for (int tile = ray_cut_unit_tile(w, u, n_tiles); tile >= 0 && tile < n_tiles;
             tile = ray_cut_next_in_unit(w, u, tile, u == cut_block && tile - u * w.block_tiles >= cut_after)) {
            if (visited >= n_tiles) return fail_noctx(NERF_ERR_INVALID, "internal error: the walk visits more tiles than the launch has");
            tiles[visited++] = tile;
        }
    return visited;
} NERF_HOST_CATCH

int nerf_debug_fine_cut_walk(int rows, int rays_per_row, int samples_per_ray, int cut_block, int cut_after, int32_t *tiles, size_t tiles_cap,
                             int32_t *blocks, int32_t *block_tiles) try {
    using namespace nerfmlp;
    if (rows <= 0 || rays_per_row <= 0 || samples_per_ray <= 0 || !tiles) return fail_noctx(NERF_ERR_INVALID, "rows, rays_per_row and samples_per_ray must be > 0, the table not NULL");
    const long long n_points = (long long)rows * rays_per_row * samples_per_ray;
    if (n_points > INT32_MAX - kPointsPerBlock) return fail_noctx(NERF_ERR_INVALID, "too many samples for one launch");
    const int n = (int)n_points, n_tiles = (n + kPointsPerBlock - 1) / kPointsPerBlock;
    if (tiles_cap < (size_t)n_tiles) return fail_noctx(NERF_ERR_INVALID, "the table holds fewer entries than the launch has tiles");
    // as the ray-mode launcher of the f32 kernels (mlp_kernel.hip launch_mlp_rays) for the ordered full launch of an image pass, then unit by
    // unit as the kernel's workgroups: a unit's first tile, then ray_cut_next_in_unit until it says the unit is finished
    const RayCutWalk w = fine_cut_walk_of(depth_order_of(n, samples_per_ray, rays_per_row, true, true).tiles, samples_per_ray, n);
    if (blocks) *blocks = w.blocks;
    if (block_tiles) *block_tiles = w.block_tiles;
    int visited = 0;
    if (w.blocks == 0) { // the launch does not qualify: it keeps the static walk (nerf_debug_tile_rotation), every tile in turn here
        for (int t = 0; t < n_tiles; ++t) tiles[visited++] = t;
        return visited;
    }
    for (int u = 0; u < ray_cut_units(w); ++u)
        for (int tile = ray_cut_unit_tile(w, u, n_tiles); tile >= 0 && tile < n_tiles;
             tile = ray_cut_next_in_unit(w, u, tile, u == cut_block && tile - u * w.block_tiles >= cut_after)) {
            if (visited >= n_tiles) return fail_noctx(NERF_ERR_INVALID, "internal error: the walk visits more tiles than the launch has");
            tiles[visited++] = tile;
        }
    return visited;
} NERF_HOST_CATCH

int nerf_debug_clip_rays(const uint32_t *occ_bits, const float lo[3], const float step[3], const int32_t dims[3], const float *origins,
                         size_t n_origins, const float *dirs, size_t n_rays, int normalize, float near_, float far_, const float *bounds,
                         float *bounds_out, uint8_t *hit_out, uint64_t *n_hit, uint64_t *n_refused_reads) try {
    const char *why = nerfclip::check_grid(occ_bits, lo, step, dims);
    if (!why) why = nerfclip::check_rays(origins, n_origins, dirs, n_rays, near_, far_, bounds, bounds_out, hit_out);
    if (why) return fail_noctx(NERF_ERR_INVALID, why);
    uint64_t hits = 0, refused = 0;
    for (size_t r = 0; r < n_rays; ++r) { // as k_clip_rays (ray_clip_kernels.hip), one ray after the other
        float near_r, far_r;
        const nerfclip::Result res = nerfclip::clip_batch_ray(occ_bits, lo, step, dims, origins, n_origins == 1 ? 0 : 1, dirs, normalize ? 1 : 0, near_, far_,
                                                              bounds, r, &near_r, &far_r);
        bounds_out[2 * r] = res.t_first; bounds_out[2 * r + 1] = res.t_last;
        hit_out[r] = res.hit ? 1 : 0;
        hits += res.hit ? 1 : 0; refused += res.refused;
    }
    if (n_hit) *n_hit = hits;
    if (n_refused_reads) *n_refused_reads = refused;
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_camera_from_json(const char *path, int width, int height, nerf_camera *out) try {
    if (!path || !out) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = camera_from_json(path, width, height, out, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

int nerf_camera_from_values(float near_, float far_, const float origin[3], const float forward[3], const float up[3],
                            const float hwf[3], int width, int height, nerf_camera *out) try {
    if (!origin || !forward || !up || !hwf || !out) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    camera_from_values(near_, far_, origin, forward, up, hwf, width, height, out);
    return NERF_OK;
} NERF_HOST_CATCH

int nerf_save_ppm(const char *path, int width, int height, const float *rgb) try {
    if (!path || !rgb) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = save_ppm(path, width, height, rgb, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

int nerf_save_pfm(const char *path, int width, int height, const float *values) try {
    if (!path || !values) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = save_pfm(path, width, height, values, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

int nerf_save_pam(const char *path, int width, int height, const uint8_t *rgba) try {
    if (!path || !rgba) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = save_pam(path, width, height, rgba, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

int nerf_save_ply(const char *path, size_t n_vertices, const float *vertices, const float *normals, const float *rgb, size_t n_triangles,
                  const uint32_t *triangles) try {
    if (!path) return fail_noctx(NERF_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = save_ply(path, n_vertices, vertices, normals, rgb, n_triangles, triangles, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

void nerf_quantize_rgb8(const float *rgb, size_t n_pixels, uint8_t *out) { quantize_rgb8(rgb, n_pixels, out); }

void nerf_quantize_rgba8(const float *rgb, size_t n_pixels, uint8_t *out) {
    for (size_t i = 0; i < n_pixels; ++i) { // no allocation: nothing here can throw across the ABI
        quantize_rgb8(rgb + 3 * i, 1, out + 4 * i);
        out[4 * i + 3] = 255;
    }
}

int nerf_check_network_blob(const char *blob_path) try {
    if (!blob_path) return fail_noctx(NERF_ERR_INVALID, "blob_path is NULL");
    std::vector<float> ws, sm;
    std::string err;
    const int rc = read_blob_file(blob_path, ws, sm, err);
    return rc ? fail_noctx(rc, err) : NERF_OK;
} NERF_HOST_CATCH

} // extern "C"
