// nerf_cli.cpp -- the MI355X counterpart of `cargo run --release` (reference src/main.rs:1-3 ->
// render_cli_image, src/lib.rs:647-677): load lego_rust/{coarse,fine}, build the camera from
// tf_reference_samples.json, render, print the same facts, write output.ppm.  Plain C++ over the C ABI
// (include/nerf_mi355x.h) -- exactly what a Rust main.rs would do through the extern "C" block of INTEGRATION.md.
//
// With no flags it reproduces the reference's run: 256x256, 64 coarse + 128 fine samples, ./output.ppm.
// --depth / --opacity add the expected-depth and opacity maps (nerf_render_image_aux) as one-channel PFM files.
// --rgba adds the display-ready frame (nerf_render_image_rgba8: packed on the device, over --background, with --alpha) as a PAM file.
// --density-grid writes the density field on a lattice (nerf_density_grid): raw little-endian f32, x fastest, and / or the occupancy words;
// with no image output asked for beside it (--out, --depth, --opacity, --rgba) the render is skipped.
// --mesh writes the level set sigma = --mesh-iso of the same lattice (--density-grid / --grid-lo / --grid-step / --grid-net) as a binary PLY with
// vertex normals (nerf_extract_mesh: marching tetrahedra on the device, the lattice never reaches the host), --mesh-colour adds vertex colours,
// --mesh-keep-largest K / --mesh-min-points M mesh only the K largest connected components of the inside points / those of at least M points.
// --rays FILE renders the caller's rays (nerf_render_rays): n x 6 little-endian f32 {origin, direction} (directions are normalised on the device),
// near / far from the scene JSON unless --rays-bounds FILE gives n x 2 {near, far}; --rays-out FILE receives n x 3 f32 linear RGB (over --background).
// --coarse / --fine / --seed / --dtype / --coarse-only apply; with no image flag beside it the render is skipped.
// --rays-normals FILE beside --rays-out adds n x 3 f32 per-ray normals (nerf_render_rays_normals; --normals-step H, default 1e-3, is the
// central-difference step).  --normals FILE.ppm writes the normal map of the image run, encoded 0.5 n + 0.5 per component: the window's rays
// (nerf_stage_ray_dirs, rng_index = row * nx + col) go through nerf_render_rays_normals once more on the first context.
// --certify-zero beside --rays renders the batch with zero certification (nerf_render_rays_certified / _clipped_certified): the same bytes, and the
// audit line of an image render.
// --rays-occupancy FILE.bits beside --rays clips the rays to the occupied cells of an occupancy grid first (nerf_render_rays_clipped): FILE holds the
// words --grid-occupancy wrote for the lattice that --density-grid / --grid-lo / --grid-step name (no grid output flag is then needed);
// --occupancy-dilate R (1..4) grows it by R cells first (nerf_occupancy_dilate).  Rays that cross no occupied cell get the background.
// --points FILE.ply writes the coloured point cloud (nerf_render_rays_points) of the --rays batch, or without --rays of the scene camera's rays
// (the window's, rng_index = row * nx + col): one vertex per ray that reaches --points-quantile Q (default 0.5, the median depth) with an opacity
// of at least --points-min-opacity A (default 0.5), with vertex normals when --normals-step H is given; a PLY with zero faces (nerf_save_ply).
// --depth-quantile FILE.pfm writes the median-depth map of the image run next to --depth (nerf_render_rays_quantiles on the window's rays).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nerf_mi355x.h"

static void usage(const char *argv0) {
    fprintf(stderr,
            "usage: %s [--scene DIR] [--width W] [--height H] [--coarse N] [--fine N] [--seed S] [--ssaa S]\n"
            "          [--coarse-only] [--crop X0,Y0,W,H] [--dtype f32|bf16|bf16x3|f16x2] [--skip-empty] [--skip-dead] [--hybrid-sampling] [--certify-zero]\n"
            "          [--device ID | --gpus N | --devices ID,ID,... [--gather host|peer|rccl]] [--frames K] [--out FILE.ppm]\n"
            "          [--depth FILE.pfm] [--opacity FILE.pfm]\n"
            "          [--rgba FILE.pam [--background R,G,B] [--alpha opaque|premultiplied|straight]]\n"
            "          [--density-grid NX,NY,NZ --grid-lo X,Y,Z --grid-step SX,SY,SZ [--grid-net coarse|fine] [--grid-threshold T]\n"
            "           [--grid-out FILE.raw] [--grid-occupancy FILE.bits] [--mesh FILE.ply [--mesh-iso V] [--mesh-colour]\n"
            "            [--mesh-keep-largest K] [--mesh-min-points M]]]\n"
            "           (at least one of the three files; no image flag: no render)\n"
            "          [--rays FILE.f32 --rays-out FILE.f32 [--rays-bounds FILE.f32] [--rays-normals FILE.f32]\n"
            "           [--rays-occupancy FILE.bits --density-grid NX,NY,NZ --grid-lo X,Y,Z --grid-step SX,SY,SZ [--occupancy-dilate R]]]\n"
            "           (n x 6 f32 in, n x 3 f32 out; no image flag: no render; --rays-occupancy: clip the rays to the grid's occupied cells first)\n"
            "          [--normals FILE.ppm] [--normals-step H]   (normal map of the image run, 0.5 n + 0.5; H: central-difference step, default 1e-3)\n"
            "          [--points FILE.ply [--points-quantile Q] [--points-min-opacity A] [--normals-step H]]\n"
            "           (the point cloud of the --rays batch, else of the camera's rays; --rays then needs no --rays-out; normals only with --normals-step)\n"
            "          [--depth-quantile FILE.pfm]   (median-depth map of the image run)\n"
            "defaults: --scene lego_rust --width 256 --height 256 --coarse 64 --fine 128 --out output.ppm --mesh-iso 10\n",
            argv0);
}

int main(int argc, char **argv) {
    std::string scene = getenv("NERF_SCENE_DIR") ? getenv("NERF_SCENE_DIR") : "lego_rust";
    std::string out = "output.ppm", depth_path, opacity_path, rgba_path;
    std::string grid_out, grid_bits_path, mesh_path, rays_path, rays_out_path, rays_bounds_path, rays_normals_path, normals_path, rays_occ_path;
    std::string points_path, depth_q_path;
    float points_quantile = 0.5f, points_min_opacity = 0.5f;
    bool have_normals_step = false;
    int occ_dilate = 0;
    float normals_step = 1e-3f;
    float mesh_iso = 10.0f;
    bool mesh_colour = false, have_mesh_opt = false;
    nerf_component_filter mesh_filter = {0, 0}; // --mesh-keep-largest / --mesh-min-points: only the kept components of the inside points are meshed
    int32_t grid_dims[3] = {0, 0, 0};
    float grid_lo[3] = {0.f, 0.f, 0.f}, grid_step[3] = {0.f, 0.f, 0.f}, grid_threshold = 0.0f;
    int grid_net = NERF_NET_FINE;
    bool want_grid = false, have_grid_lo = false, have_grid_step = false, want_image = false;
    float background[3] = {1.0f, 1.0f, 1.0f};
    bool have_background = false;
    int alpha_mode = NERF_ALPHA_OPAQUE;
    int width = 256, height = 256, device = 0, frames = 1, gpus = 1, gather = NERF_GATHER_HOST; // src/lib.rs:657-658
    std::vector<int> devices;
    nerf_render_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.n_coarse = 64; opts.n_fine = 128; // default_sample_counts, src/lib.rs:603-612
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { usage(argv[0]); exit(2); } return argv[++i]; };
        if (a == "--scene") scene = next();
        else if (a == "--width") width = atoi(next());
        else if (a == "--height") height = atoi(next());
        else if (a == "--coarse") opts.n_coarse = atoi(next());
        else if (a == "--fine") opts.n_fine = atoi(next());
        else if (a == "--seed") opts.seed = strtoull(next(), nullptr, 10);
        else if (a == "--ssaa") opts.ssaa = atoi(next());
        else if (a == "--coarse-only") opts.coarse_only = 1;
        else if (a == "--dtype") { const std::string d = next(); if (d == "bf16") opts.mlp_dtype = NERF_MLP_BF16; else if (d == "bf16x3") opts.mlp_dtype = NERF_MLP_BF16X3; else if (d == "f16x2") opts.mlp_dtype = NERF_MLP_F16X2; else if (d != "f32") { usage(argv[0]); return 2; } }
        else if (a == "--skip-empty") opts.skip_empty = 1;
        else if (a == "--skip-dead") opts.skip_dead = 1;
        else if (a == "--hybrid-sampling") opts.hybrid_sampling = 1;
        else if (a == "--certify-zero") opts.certify_zero = 1;
        else if (a == "--gpus") gpus = atoi(next());
        else if (a == "--devices") { // explicit device list, one context each (ids may repeat: several contexts on one GPU)
            devices.clear();
            for (const char *p = next(); *p;) { devices.push_back((int)strtol(p, (char **)&p, 10)); if (*p == ',') ++p; else if (*p) { usage(argv[0]); return 2; } }
            gpus = (int)devices.size();
        }
        else if (a == "--gather") { const std::string g = next(); gather = g == "peer" ? NERF_GATHER_PEER : g == "rccl" ? NERF_GATHER_RCCL : NERF_GATHER_HOST; }
        else if (a == "--device") device = atoi(next());
        else if (a == "--frames") frames = atoi(next());
        else if (a == "--out") { out = next(); want_image = true; }
        else if (a == "--depth") { depth_path = next(); want_image = true; }
        else if (a == "--opacity") { opacity_path = next(); want_image = true; }
        else if (a == "--rgba") { rgba_path = next(); want_image = true; }
        else if (a == "--density-grid") {
            if (sscanf(next(), "%d,%d,%d", &grid_dims[0], &grid_dims[1], &grid_dims[2]) != 3) { usage(argv[0]); return 2; }
            want_grid = true;
        }
        else if (a == "--grid-lo") { if (sscanf(next(), "%f,%f,%f", &grid_lo[0], &grid_lo[1], &grid_lo[2]) != 3) { usage(argv[0]); return 2; } have_grid_lo = true; }
        else if (a == "--grid-step") { if (sscanf(next(), "%f,%f,%f", &grid_step[0], &grid_step[1], &grid_step[2]) != 3) { usage(argv[0]); return 2; } have_grid_step = true; }
        else if (a == "--grid-net") { const std::string n = next(); if (n == "coarse") grid_net = NERF_NET_COARSE; else if (n == "fine") grid_net = NERF_NET_FINE; else { usage(argv[0]); return 2; } }
        else if (a == "--grid-threshold") grid_threshold = strtof(next(), nullptr);
        else if (a == "--grid-out") grid_out = next();
        else if (a == "--grid-occupancy") grid_bits_path = next();
        else if (a == "--mesh") mesh_path = next();
        else if (a == "--rays") rays_path = next();
        else if (a == "--rays-out") rays_out_path = next();
        else if (a == "--rays-bounds") rays_bounds_path = next();
        else if (a == "--rays-normals") rays_normals_path = next();
        else if (a == "--rays-occupancy") rays_occ_path = next();
        else if (a == "--occupancy-dilate") occ_dilate = atoi(next());
        else if (a == "--normals") { normals_path = next(); want_image = true; }
        else if (a == "--normals-step") { normals_step = strtof(next(), nullptr); have_normals_step = true; }
        else if (a == "--points") points_path = next();
        else if (a == "--points-quantile") points_quantile = strtof(next(), nullptr);
        else if (a == "--points-min-opacity") points_min_opacity = strtof(next(), nullptr);
        else if (a == "--depth-quantile") { depth_q_path = next(); want_image = true; }
        else if (a == "--mesh-iso") { mesh_iso = strtof(next(), nullptr); have_mesh_opt = true; }
        else if (a == "--mesh-colour") { mesh_colour = true; have_mesh_opt = true; }
        else if (a == "--mesh-keep-largest") { mesh_filter.keep_largest = (uint32_t)strtoul(next(), nullptr, 10); have_mesh_opt = true; }
        else if (a == "--mesh-min-points") { mesh_filter.min_points = (uint32_t)strtoul(next(), nullptr, 10); have_mesh_opt = true; }
        else if (a == "--background") {
            if (sscanf(next(), "%f,%f,%f", &background[0], &background[1], &background[2]) != 3) { usage(argv[0]); return 2; }
            have_background = true;
        }
        else if (a == "--alpha") {
            const std::string m = next();
            if (m == "opaque") alpha_mode = NERF_ALPHA_OPAQUE; else if (m == "premultiplied") alpha_mode = NERF_ALPHA_PREMULTIPLIED;
            else if (m == "straight") alpha_mode = NERF_ALPHA_STRAIGHT; else { usage(argv[0]); return 2; }
        }
        else if (a == "--crop") {
            if (sscanf(next(), "%d,%d,%d,%d", &opts.crop_x0, &opts.crop_y0, &opts.crop_w, &opts.crop_h) != 4) { usage(argv[0]); return 2; }
        } else { usage(argv[0]); return a == "--help" || a == "-h" ? 0 : 2; }
    }

    const bool grid_files = !(grid_out.empty() && grid_bits_path.empty() && mesh_path.empty());
    if (want_grid && (!have_grid_lo || !have_grid_step || (!grid_files && rays_occ_path.empty()))) { usage(argv[0]); return 2; }
    // --rays-occupancy: the lattice flags describe the file's grid; it goes with --rays, not with normals; --occupancy-dilate goes with it
    if (!rays_occ_path.empty() && (rays_path.empty() || !want_grid || !rays_normals_path.empty())) { usage(argv[0]); return 2; }
    if (occ_dilate != 0 && (rays_occ_path.empty() || occ_dilate < 1 || occ_dilate > 4)) { usage(argv[0]); return 2; }
    if (!want_grid && (have_grid_lo || have_grid_step || !grid_out.empty() || !grid_bits_path.empty() || !mesh_path.empty())) { usage(argv[0]); return 2; }
    if (mesh_path.empty() && have_mesh_opt) { usage(argv[0]); return 2; }
    if (rays_path.empty() ? !(rays_out_path.empty() && rays_bounds_path.empty() && rays_normals_path.empty()) : (rays_out_path.empty() && points_path.empty())) { usage(argv[0]); return 2; }
    if (rays_out_path.empty() && !(rays_normals_path.empty() && rays_occ_path.empty())) { usage(argv[0]); return 2; }

    // one context per GPU (--gpus N: devices 0..N-1, the rayon fan-out of src/lib.rs:533-550 becomes a fan-out over devices)
    if (gpus < 1) { usage(argv[0]); return 2; }
    std::vector<nerf_ctx *> ctxs(gpus, nullptr);
    if (gpus == 1 && devices.empty() ? nerf_create(device, &ctxs[0]) : nerf_create_multi(devices.empty() ? nullptr : devices.data(), gpus, ctxs.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; }
    nerf_ctx *ctx = ctxs[0];
    for (nerf_ctx *c : ctxs)
        if (nerf_load_network_dir(c, NERF_NET_COARSE, (scene + "/coarse").c_str()) ||
            nerf_load_network_dir(c, NERF_NET_FINE, (scene + "/fine").c_str())) {
            fprintf(stderr, "error: %s\n", nerf_last_error(c));
            return 1;
        }
    // --points: the cloud of a batch on the first context into a PLY without faces (a batch keeps at most one point per ray)
    auto write_points = [&](const float *origins, size_t n_origins, const float *dirs, size_t n, int normalize, float near_, float far_, const float *bounds,
                            const uint32_t *index, const nerf_render_opts &ro) {
        const float h = have_normals_step ? normals_step : 0.0f;
        std::vector<float> xyz(3 * n + 1), colour(3 * n + 1), nrm(h > 0.0f ? 3 * n + 1 : 0);
        size_t kept = 0;
        nerf_stats pst;
        if (nerf_render_rays_points(ctx, origins, n_origins, dirs, n, normalize, near_, far_, bounds, index, &ro, points_quantile, points_min_opacity, h, n,
                                    xyz.data(), colour.data(), nrm.empty() ? nullptr : nrm.data(), nullptr, nullptr, nullptr, &kept, &pst)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return false;
        }
        if (nerf_save_ply(points_path.c_str(), kept, xyz.data(), nrm.empty() ? nullptr : nrm.data(), colour.data(), 0, nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(nullptr));
            return false;
        }
        printf("point cloud at quantile %g, opacity >= %g: %zu of %zu rays kept%s: device %.2f ms in %u pass(es)\n", (double)points_quantile, (double)points_min_opacity,
               kept, n, nrm.empty() ? "" : ", with normals", n ? pst.ms_total : 0.0, n ? pst.n_passes : 0u);
        return true;
    };
    // the window's rays as a batch (nerf_stage_ray_dirs, rng_index = row * nx + col): what --normals, --points and --depth-quantile render
    auto window_batch = [&](const nerf_camera &cam, std::vector<float> &dirs, std::vector<uint32_t> &index, nerf_render_opts &ro) {
        const int ow = opts.crop_w > 0 ? opts.crop_w : width, oh = opts.crop_h > 0 ? opts.crop_h : height;
        const int x0 = opts.crop_w > 0 ? opts.crop_x0 : 0, y0 = opts.crop_h > 0 ? opts.crop_y0 : 0;
        dirs.resize(3 * (size_t)ow * oh); index.resize((size_t)ow * oh);
        for (int i = 0; i < oh; ++i)
            for (int j = 0; j < ow; ++j) index[(size_t)i * ow + j] = (uint32_t)(y0 + i) * (uint32_t)width + (uint32_t)(x0 + j);
        ro = opts; // ray batches have no pixel grid; what else they refuse (ssaa, the skip modes) is the library's error
        ro.crop_x0 = ro.crop_y0 = ro.crop_w = ro.crop_h = 0;
        if (nerf_stage_ray_dirs(ctx, &cam, x0, y0, ow, oh, 1, dirs.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(ctx)); return false; }
        return true;
    };
    if (!rays_path.empty()) { // the caller's rays on the first context
        auto slurp = [](const std::string &path, std::vector<float> &v) { // the host is little-endian: the bytes as they are
            FILE *f = fopen(path.c_str(), "rb");
            if (!f) return false;
            bool ok = fseek(f, 0, SEEK_END) == 0;
            const long bytes = ok ? ftell(f) : -1;
            ok = ok && bytes >= 0 && bytes % (long)sizeof(float) == 0 && fseek(f, 0, SEEK_SET) == 0;
            if (ok) { v.resize((size_t)bytes / sizeof(float)); ok = fread(v.data(), 1, (size_t)bytes, f) == (size_t)bytes; }
            fclose(f);
            return ok;
        };
        std::vector<float> rays, ray_bounds;
        if (!slurp(rays_path, rays) || rays.size() % 6 != 0) { fprintf(stderr, "error: %s must hold n x 6 f32 (origin, direction)\n", rays_path.c_str()); return 1; }
        const size_t n = rays.size() / 6;
        if (!rays_bounds_path.empty() && (!slurp(rays_bounds_path, ray_bounds) || ray_bounds.size() != 2 * n)) {
            fprintf(stderr, "error: %s must hold n x 2 f32 (near, far), one pair per ray of %s\n", rays_bounds_path.c_str(), rays_path.c_str());
            return 1;
        }
        nerf_camera jc; // near and far of the scene
        if (nerf_camera_from_json((scene + "/tf_reference_samples.json").c_str(), width, height, &jc)) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; }
        std::vector<float> o(3 * n), d(3 * n), rgb(3 * n), normals(rays_normals_path.empty() ? 0 : 3 * n + 1); // + 1: never a NULL pointer, also for n = 0
        for (size_t r = 0; r < n; ++r)
            for (int k = 0; k < 3; ++k) { o[3 * r + k] = rays[6 * r + k]; d[3 * r + k] = rays[6 * r + 3 + k]; }
        nerf_stats rst;
        const float *rb = ray_bounds.empty() ? nullptr : ray_bounds.data(), *bg = have_background ? background : nullptr;
        uint64_t n_hit = 0;
        std::vector<uint32_t> occ;
        if (!rays_occ_path.empty()) { // the occupancy words of the lattice the grid flags name, grown on request
            const bool ok_dims = grid_dims[0] > 0 && grid_dims[1] > 0 && grid_dims[2] > 0;
            const unsigned long long cells = ok_dims ? (unsigned long long)grid_dims[0] * (unsigned long long)grid_dims[1] * (unsigned long long)grid_dims[2] : 0;
            if (!ok_dims || cells > 0x7fffffffull) { fprintf(stderr, "error: --density-grid must name at most 2^31 - 1 cells\n"); return 1; }
            FILE *f = fopen(rays_occ_path.c_str(), "rb");
            occ.resize((size_t)((cells + 31) / 32));
            const bool ok = f && fread(occ.data(), sizeof(uint32_t), occ.size(), f) == occ.size() && fgetc(f) == EOF;
            if (f) fclose(f);
            if (!ok) {
                fprintf(stderr, "error: %s must hold the %zu occupancy words of a %d x %d x %d grid\n", rays_occ_path.c_str(), occ.size(), grid_dims[0], grid_dims[1], grid_dims[2]);
                return 1;
            }
            if (occ_dilate) {
                std::vector<uint32_t> grown(occ.size());
                if (nerf_occupancy_dilate(ctx, occ.data(), grid_dims, occ_dilate, grown.data(), nullptr, nullptr)) { fprintf(stderr, "error: %s\n", nerf_last_error(ctx)); return 1; }
                occ.swap(grown);
            }
        }
        if (!points_path.empty() && !write_points(o.data(), n, d.data(), n, 1, jc.near_, jc.far_, rb, nullptr, opts)) return 1;
        if (rays_out_path.empty()) {
            if (!want_image && !want_grid) {
                for (nerf_ctx *c : ctxs) nerf_destroy(c);
                return 0;
            }
        } else {
            const bool certified = opts.certify_zero != 0; // --certify-zero: the certified forms of the two calls, the same bytes in --rays-out
            if (certified && !normals.empty()) { fprintf(stderr, "error: --rays-normals is not offered with --certify-zero\n"); return 1; }
            if (!occ.empty() ? (certified ? nerf_render_rays_clipped_certified : nerf_render_rays_clipped)(ctx, occ.data(), grid_lo, grid_step, grid_dims, o.data(), n, d.data(), n, 1,
                                                        jc.near_, jc.far_, rb, nullptr, &opts, bg, rgb.data(), nullptr, nullptr, nullptr, &n_hit, &rst)
                : certified ? nerf_render_rays_certified(ctx, o.data(), n, d.data(), n, 1, jc.near_, jc.far_, rb, nullptr, &opts, bg, rgb.data(), nullptr, nullptr, &rst)
                : normals.empty() ? nerf_render_rays(ctx, o.data(), n, d.data(), n, 1, jc.near_, jc.far_, rb, nullptr, &opts, bg, rgb.data(), nullptr, nullptr, &rst)
                                : nerf_render_rays_normals(ctx, o.data(), n, d.data(), n, 1, jc.near_, jc.far_, rb, nullptr, &opts, bg, rgb.data(), nullptr, nullptr,
                                                           normals_step, normals.data(), &rst)) {
                fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
                return 1;
            }
            auto put = [](const std::string &path, const float *v, size_t count) {
                FILE *f = fopen(path.c_str(), "wb");
                const bool ok = f && fwrite(v, sizeof(float), count, f) == count;
                if ((f && fclose(f)) || !ok) { fprintf(stderr, "error: cannot write %s\n", path.c_str()); return false; }
                return true;
            };
            if (!put(rays_out_path, rgb.data(), rgb.size())) return 1;
            if (!normals.empty() && !put(rays_normals_path, normals.data(), 3 * n)) return 1;
            if (!occ.empty()) { // the stats are those of the compacted batch
                printf("%zu rays, %llu of them cross an occupied cell (%d coarse + %d fine samples): device %.2f ms in %u pass(es)\n", n, (unsigned long long)n_hit,
                       opts.n_coarse, opts.coarse_only ? 0 : opts.n_fine, n_hit ? rst.ms_total : 0.0, n_hit ? rst.n_passes : 0u);
                if (!grid_files) want_grid = false; // the lattice flags only described the occupancy file
            } else
                printf("%zu rays (%d coarse + %d fine samples): device %.2f ms in %u pass(es)\n", n, opts.n_coarse, opts.coarse_only ? 0 : opts.n_fine, n ? rst.ms_total : 0.0,
                       n ? rst.n_passes : 0u);
            if (certified && (occ.empty() ? n > 0 : n_hit > 0)) // the audit of the batch, as an image render prints it below
                printf("certify_zero audit: %llu certificates evaluated all the same, %llu violations, margins %.3g / %.3g, least headroom %.3g / %.3g, largest bf16 error %.3g / %.3g, "
                       "batch rendered again %u time(s), %u rays beyond their predicted cut\n", (unsigned long long)rst.n_certify_audited, (unsigned long long)rst.n_certify_violations,
                       (double)rst.certify_margin[0], (double)rst.certify_margin[1], (double)rst.certify_headroom[0], (double)rst.certify_headroom[1],
                       (double)rst.certify_max_error[0], (double)rst.certify_max_error[1], rst.n_certify_retries, rst.n_certify_fallback_rays);
            if (!want_image && !want_grid) {
                for (nerf_ctx *c : ctxs) nerf_destroy(c);
                return 0;
            }
        }
    }
    if (want_grid && !mesh_path.empty()) { // the level set of the lattice as a mesh: size query, then the fill (the lattice is evaluated twice)
        uint64_t nv = 0, nt = 0, n_comp = 0, n_kept = 0;
        const bool filtered = mesh_filter.keep_largest || mesh_filter.min_points;
        const nerf_component_filter *filter = filtered ? &mesh_filter : nullptr; // no filter: the unfiltered path, no labelling
        if (nerf_extract_mesh_filtered(ctx, grid_net, grid_lo, grid_step, grid_dims, mesh_iso, filter, nullptr, nullptr, nullptr, 0, nullptr, 0, &nv, &nt,
                                       filtered ? &n_comp : nullptr, filtered ? &n_kept : nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        std::vector<float> verts(3 * (size_t)nv), normals(3 * (size_t)nv), colours(mesh_colour ? 3 * (size_t)nv : 0);
        std::vector<uint32_t> tris(3 * (size_t)nt);
        if (nv && nerf_extract_mesh_filtered(ctx, grid_net, grid_lo, grid_step, grid_dims, mesh_iso, filter, verts.data(), normals.data(),
                                             mesh_colour ? colours.data() : nullptr, (size_t)nv, tris.data(), (size_t)nt, &nv, &nt, nullptr, nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        if (nerf_save_ply(mesh_path.c_str(), (size_t)nv, verts.data(), normals.data(), mesh_colour ? colours.data() : nullptr, (size_t)nt, tris.data())) {
            fprintf(stderr, "error: %s\n", nerf_last_error(nullptr));
            return 1;
        }
        printf("mesh sigma = %g on %d x %d x %d (%s network): %llu vertices, %llu triangles\n", (double)mesh_iso, grid_dims[0], grid_dims[1], grid_dims[2],
               grid_net == NERF_NET_FINE ? "fine" : "coarse", (unsigned long long)nv, (unsigned long long)nt);
        if (filtered)
            printf("components of sigma > %g (keep largest %u, at least %u points): %llu components, %llu kept\n", (double)mesh_iso, mesh_filter.keep_largest,
                   mesh_filter.min_points, (unsigned long long)n_comp, (unsigned long long)n_kept);
        if (grid_out.empty() && grid_bits_path.empty()) {
            if (!want_image) {
                for (nerf_ctx *c : ctxs) nerf_destroy(c);
                return 0;
            }
            want_grid = false;
        }
    }
    if (want_grid) { // the density field on the first context (one launch, one GPU)
        const bool ok_dims = grid_dims[0] > 0 && grid_dims[1] > 0 && grid_dims[2] > 0;
        const size_t cells = ok_dims ? (size_t)grid_dims[0] * (size_t)grid_dims[1] * (size_t)grid_dims[2] : 0; // the library refuses bad dims and sizes beyond one launch
        std::vector<float> sigma;
        std::vector<uint32_t> bits;
        if (ok_dims && cells < ((size_t)1 << 31)) {
            if (!grid_out.empty()) sigma.resize(cells);
            if (!grid_bits_path.empty()) bits.resize((cells + 31) / 32);
        }
        uint64_t occupied = 0;
        int32_t bounds[6] = {0, 0, 0, 0, 0, 0};
        if (nerf_density_grid(ctx, grid_net, grid_lo, grid_step, grid_dims, sigma.empty() ? nullptr : sigma.data(), grid_threshold,
                              bits.empty() ? nullptr : bits.data(), bits.empty() ? nullptr : &occupied, bits.empty() ? nullptr : bounds)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        auto dump = [](const std::string &path, const void *data, size_t bytes) { // the host is little-endian: the bytes as they are
            FILE *f = fopen(path.c_str(), "wb");
            const bool ok = f && fwrite(data, 1, bytes, f) == bytes;
            if (f && fclose(f)) return false;
            return ok;
        };
        if (!sigma.empty() && !dump(grid_out, sigma.data(), sigma.size() * sizeof(float))) { fprintf(stderr, "error: cannot write %s\n", grid_out.c_str()); return 1; }
        if (!bits.empty() && !dump(grid_bits_path, bits.data(), bits.size() * sizeof(uint32_t))) { fprintf(stderr, "error: cannot write %s\n", grid_bits_path.c_str()); return 1; }
        printf("density grid %d x %d x %d (%s network): %zu cells", grid_dims[0], grid_dims[1], grid_dims[2], grid_net == NERF_NET_FINE ? "fine" : "coarse", cells);
        if (!bits.empty())
            printf(", %llu with sigma > %g, index bounds x %d..%d y %d..%d z %d..%d", (unsigned long long)occupied, (double)grid_threshold,
                   bounds[0], bounds[3], bounds[1], bounds[4], bounds[2], bounds[5]);
        printf("\n");
        if (!want_image) {
            for (nerf_ctx *c : ctxs) nerf_destroy(c);
            return 0;
        }
    }
    nerf_camera cam;
    if (nerf_camera_from_json((scene + "/tf_reference_samples.json").c_str(), width, height, &cam)) {
        fprintf(stderr, "error: %s\n", nerf_last_error(nullptr));
        return 1;
    }
    if (!points_path.empty() && rays_path.empty()) { // the camera's rays; with no image flag beside it the render is skipped
        std::vector<float> dirs;
        std::vector<uint32_t> index;
        nerf_render_opts ro;
        if (!window_batch(cam, dirs, index, ro) || !write_points(cam.pos, 1, dirs.data(), index.size(), 0, cam.near_, cam.far_, nullptr, index.data(), ro)) return 1;
        if (!want_image) {
            for (nerf_ctx *c : ctxs) nerf_destroy(c);
            return 0;
        }
    }
    printf("Rendering with %d coarse samples and %d fine samples per ray\n", opts.n_coarse, opts.n_fine); // :660-663
    const int ow = opts.crop_w > 0 ? opts.crop_w : width, oh = opts.crop_h > 0 ? opts.crop_h : height;
    std::vector<float> image((size_t)ow * oh * 3);
    std::vector<float> depth(depth_path.empty() ? 0 : (size_t)ow * oh), opacity(opacity_path.empty() ? 0 : (size_t)ow * oh);
    float *d_map = depth.empty() ? nullptr : depth.data(), *o_map = opacity.empty() ? nullptr : opacity.data();
    printf("Starting image rendering...\n"); // :667
    nerf_stats st;
    std::vector<nerf_stats> per(gpus);
    double best = 1e30;
    for (int f = 0; f < frames; ++f) {
        const auto t0 = std::chrono::steady_clock::now(); // Instant::now() :668
        if (gpus == 1 ? nerf_render_image_aux(ctx, &cam, &opts, image.data(), d_map, o_map, &st)
                      : nerf_render_image_multi_aux(ctxs.data(), gpus, &cam, &opts, gather, image.data(), d_map, o_map, per.data())) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        if (gpus > 1) { // whole-job view: rays add up, device time is the slowest band's
            st = per[0];
            for (int g = 1; g < gpus; ++g) {
                st.n_rays += per[g].n_rays;
                st.n_nonfinite_points += per[g].n_nonfinite_points;
                if (per[g].ms_total > st.ms_total) { st.ms_total = per[g].ms_total; st.ms_coarse_mlp = per[g].ms_coarse_mlp; st.ms_fine_mlp = per[g].ms_fine_mlp; st.ms_other = per[g].ms_other; }
            }
        }
        if (st.n_nonfinite_points) { // a split arithmetic left its range (f16x2: an activation beyond 65 504): the image is wrong there
            fprintf(stderr, "error: %llu evaluations left the range of the selected arithmetic (nerf_stats.n_nonfinite_points); use --dtype bf16x3 or f32\n",
                    (unsigned long long)st.n_nonfinite_points);
            return 1;
        }
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        best = secs < best ? secs : best;
        printf("Rendering complete: %llu/%llu pixels (100.0%%)\n", (unsigned long long)ow * oh, (unsigned long long)ow * oh); // :559-562
        printf("Rendering completed in %.2f seconds\n", secs); // :672-675
    }
    int n_cus = 0; char arch[64] = {0};
    nerf_device_info(ctx, &n_cus, arch, sizeof arch);
    // FLOPs per point as EXECUTED by the f32 kernels (bottleneck folded into viewdirs at load time: 2 x 256 x 256 fewer than the
    // reference's graph).  The 16-bit arithmetics still execute the unfolded head: their full evaluations are priced 11 % low.
    const double kFlopPerPointFull = 1055744.0, kFlopPerPointFullReferenceGraph = 1186816.0, kFlopPerPointSigma = 982528.0;
    (void)kFlopPerPointFullReferenceGraph;
    const double flop_ray = opts.coarse_only ? opts.n_coarse * kFlopPerPointFull
                                             : opts.n_coarse * kFlopPerPointSigma + (double)(opts.n_coarse + opts.n_fine) * kFlopPerPointFull;
    const bool bf16 = opts.mlp_dtype != NERF_MLP_F32;
    const double mfma_flops = opts.mlp_dtype == NERF_MLP_BF16X3 ? 6.0 : opts.mlp_dtype == NERF_MLP_F16X2 ? 3.0 : 1.0; // executed bf16 MFMA flops per algorithmic f32 flop
    if (gpus > 1) printf("%d GPUs, %s gathered by %s\n", gpus, (opts.skip_dead || opts.skip_empty || opts.certify_zero) ? "rows dealt out round-robin," : "contiguous row bands", gather == NERF_GATHER_PEER ? "xGMI peer copies" : gather == NERF_GATHER_RCCL ? "one RCCL all-gather" : "direct D2H");
    const bool skips = opts.skip_dead || opts.skip_empty || opts.certify_zero; // then less than the algorithmic work is executed: not a roofline fraction
    printf("device %s (%d CUs): %.0f rays/s (best of %d, host wall incl. D2H); device %.1f ms = coarse MLP %.1f + fine MLP %.1f + other %.1f; "
           "%s%.1f%% of the %s MFMA roofline%s\n",
           arch, n_cus, (double)st.n_rays / best, frames, st.ms_total, st.ms_coarse_mlp, st.ms_fine_mlp, st.ms_other,
           skips ? "the ALGORITHMIC work of these rays per second = " : "",
           100.0 * mfma_flops * (double)st.n_rays * flop_ray / (st.ms_total * 1e-3) / (gpus * (bf16 ? 2500e12 : 157.3e12)),
           bf16 ? "2.5 PFLOP/s bf16" : "157.3 TFLOP/s fp32", skips ? " (work provably without effect is skipped: not a utilisation figure)" : "");
    if (opts.certify_zero) // the audit of the last frame (first context): what the certificates rested on
        printf("certify_zero audit: %llu certificates evaluated all the same, %llu violations, margins %.3g / %.3g, least headroom %.3g / %.3g, largest bf16 error %.3g / %.3g, "
               "frame rendered again %u time(s), %u rays beyond their predicted cut\n", (unsigned long long)st.n_certify_audited, (unsigned long long)st.n_certify_violations,
               (double)st.certify_margin[0], (double)st.certify_margin[1], (double)st.certify_headroom[0], (double)st.certify_headroom[1],
               (double)st.certify_max_error[0], (double)st.certify_max_error[1], st.n_certify_retries, st.n_certify_fallback_rays);
    if (nerf_save_ppm(out.c_str(), ow, oh, image.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; } // :676
    if (!rgba_path.empty()) { // the same frame once more, display-ready: packed on the device, 4 bytes per pixel come back
        std::vector<uint8_t> rgba((size_t)ow * oh * 4);
        const float *bg = have_background ? background : nullptr;
        if (gpus == 1 ? nerf_render_image_rgba8(ctx, &cam, &opts, bg, alpha_mode, rgba.data(), nullptr)
                      : nerf_render_image_multi_rgba8(ctxs.data(), gpus, &cam, &opts, gather, bg, alpha_mode, rgba.data(), nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        if (nerf_save_pam(rgba_path.c_str(), ow, oh, rgba.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; }
    }
    if ((d_map && nerf_save_pfm(depth_path.c_str(), ow, oh, d_map)) || (o_map && nerf_save_pfm(opacity_path.c_str(), ow, oh, o_map))) {
        fprintf(stderr, "error: %s\n", nerf_last_error(nullptr));
        return 1;
    }
    if (!depth_q_path.empty()) { // the median depth of the window's rays, next to the expected depth above
        std::vector<float> dirs;
        std::vector<uint32_t> index;
        nerf_render_opts ro;
        if (!window_batch(cam, dirs, index, ro)) return 1;
        const size_t n = index.size();
        const float median = 0.5f;
        std::vector<float> rgb(3 * n), depth_q(n);
        if (nerf_render_rays_quantiles(ctx, cam.pos, 1, dirs.data(), n, 0, cam.near_, cam.far_, nullptr, index.data(), &ro, nullptr, rgb.data(), nullptr, nullptr,
                                       &median, 1, depth_q.data(), nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        if (nerf_save_pfm(depth_q_path.c_str(), ow, oh, depth_q.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; }
    }
    if (!normals_path.empty()) { // the window's rays as a batch: colour as the frame above, plus the normals (there is no image entry point for them)
        const int x0 = opts.crop_w > 0 ? opts.crop_x0 : 0, y0 = opts.crop_h > 0 ? opts.crop_y0 : 0;
        const size_t n = (size_t)ow * oh;
        std::vector<float> dirs(3 * n), rgb(3 * n), normals(3 * n);
        std::vector<uint32_t> index(n);
        for (int i = 0; i < oh; ++i)
            for (int j = 0; j < ow; ++j) index[(size_t)i * ow + j] = (uint32_t)(y0 + i) * (uint32_t)width + (uint32_t)(x0 + j);
        nerf_render_opts ro = opts; // ray batches have no pixel grid; what else they refuse (ssaa, the skip modes) is the library's error
        ro.crop_x0 = ro.crop_y0 = ro.crop_w = ro.crop_h = 0;
        if (nerf_stage_ray_dirs(ctx, &cam, x0, y0, ow, oh, 1, dirs.data()) ||
            nerf_render_rays_normals(ctx, cam.pos, 1, dirs.data(), n, 0, cam.near_, cam.far_, nullptr, index.data(), &ro, nullptr, rgb.data(), nullptr, nullptr,
                                     normals_step, normals.data(), nullptr)) {
            fprintf(stderr, "error: %s\n", nerf_last_error(ctx));
            return 1;
        }
        for (float &v : normals) v = 0.5f * v + 0.5f; // a zero normal (a ray that met nothing) becomes mid grey
        if (nerf_save_ppm(normals_path.c_str(), ow, oh, normals.data())) { fprintf(stderr, "error: %s\n", nerf_last_error(nullptr)); return 1; }
    }
    for (nerf_ctx *c : ctxs) nerf_destroy(c);
    return 0;
}
