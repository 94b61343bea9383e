//! Raw bindings to libnerf_mi355x.so.  One-to-one with include/nerf_mi355x.h (ABI version 5): every function the header
//! declares is declared here with the same number of arguments (tests/test_host_logic.py parses both and compares);
//! layouts are `#[repr(C)]` mirrors of `nerf_camera`, `nerf_render_opts`, `nerf_stats` -- call `check_layouts()` once at
//! start-up to compare their sizes with the library's (`nerf_abi_struct_sizes`).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct nerf_ctx {
    _private: [u8; 0],
}

/// `struct Camera` of the reference (src/lib.rs:197-211); `samples_per_ray` lives in `nerf_render_opts::n_coarse`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct nerf_camera {
    pub nx: i32,
    pub ny: i32,
    pub alpha_width: f32,
    pub alpha_height: f32,
    pub pos: [f32; 3],
    pub dir: [f32; 3],
    pub up: [f32; 3],
    pub near: f32,
    pub far: f32,
}

/// `nerf_render_opts::mlp_dtype` / `nerf_forward_batch_ex`: the MLP arithmetic (include/nerf_mi355x.h).
pub const NERF_MLP_F32: i32 = 0;
pub const NERF_MLP_BF16: i32 = 1;
pub const NERF_MLP_BF16X3: i32 = 2;
pub const NERF_MLP_F16X2: i32 = 3;
/// `nerf_debug_network_stream_dir`'s `kind`: which 16-bit weight stream.
pub const NERF_STREAM_BF16V2: c_int = 0;
pub const NERF_STREAM_F16V2: c_int = 1;
pub const NERF_STREAM_BF16X3: c_int = 2;
pub const NERF_STREAM_F16X2: c_int = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct nerf_render_opts {
    pub n_coarse: i32,
    pub n_fine: i32,
    pub coarse_only: i32,
    pub crop_x0: i32,
    pub crop_y0: i32,
    pub crop_w: i32,
    pub crop_h: i32,
    pub ssaa: i32,
    pub seed: u64,
    pub mlp_dtype: i32,
    pub skip_empty: i32,
    pub skip_dead: i32,
    pub hybrid_sampling: i32,
    pub certify_zero: i32,
    pub band_index: i32,
    pub band_count: i32,
    pub band_stripe_rows: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct nerf_stats {
    pub n_rays: u64,
    pub n_coarse_points: u64,
    pub n_fine_points: u64,
    pub ms_total: f64,
    pub ms_coarse_mlp: f64,
    pub ms_fine_mlp: f64,
    pub ms_other: f64,
    pub n_mlp_launches: u32,
    pub n_passes: u32,
    pub n_colour_skipped_points: u64,
    pub n_exec_coarse_trunk: u64,
    pub n_exec_fine_trunk: u64,
    pub n_exec_colour: u64,
    pub n_hybrid_rays: u64,
    pub n_nonfinite_points: u64,
    pub n_certify_audited: u64,
    pub n_certify_violations: u64,
    pub n_certify_retries: u32,
    pub n_certify_fallback_rays: u32,
    pub certify_margin: [f32; 2],
    pub certify_headroom: [f32; 2],
    pub certify_max_error: [f32; 2],
}

/// `filter` of the `*_filtered` mesh entry points ("lattice components" in include/nerf_mi355x.h): a component of the inside points is kept
/// iff `n_points >= min_points` and (`keep_largest == 0` or its rank < `keep_largest`); `keep_largest` <= 64.  Passed as `*const c_void`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct nerf_component_filter {
    pub keep_largest: u32,
    pub min_points: u32,
}

/// One entry of `nerf_lattice_components`' table (passed as `*mut c_void`): `label` = the smallest linear index of the component,
/// `bounds` = inclusive {ix_min, iy_min, iz_min, ix_max, iy_max, iz_max}.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct nerf_component {
    pub label: u32,
    pub n_points: u32,
    pub bounds: [i32; 6],
}

/// `gather` of `nerf_render_image_multi`
pub const NERF_GATHER_HOST: c_int = 0;
pub const NERF_GATHER_PEER: c_int = 1;
pub const NERF_GATHER_RCCL: c_int = 2;

/// `alpha_mode` of `nerf_render_image_rgba8`: colour over the background with alpha 255; premultiplied colour + opacity; colour / opacity + opacity
pub const NERF_ALPHA_OPAQUE: c_int = 0;
pub const NERF_ALPHA_PREMULTIPLIED: c_int = 1;
pub const NERF_ALPHA_STRAIGHT: c_int = 2;

pub const NERF_OK: c_int = 0;
pub const NERF_ERR_INVALID: c_int = -1;
pub const NERF_ERR_IO: c_int = -2;
pub const NERF_ERR_MISSING: c_int = -3;
pub const NERF_ERR_SHAPE: c_int = -4;
pub const NERF_ERR_HIP: c_int = -5;
pub const NERF_ERR_STATE: c_int = -6;
pub const NERF_ERR_PARSE: c_int = -7;
pub const NERF_NET_COARSE: c_int = 0;
pub const NERF_NET_FINE: c_int = 1;

extern "C" {
    pub fn nerf_abi_version() -> c_int;
    pub fn nerf_build_variant() -> *const c_char;
    pub fn nerf_abi_struct_sizes(camera: *mut usize, render_opts: *mut usize, stats: *mut usize);
    pub fn nerf_create(device_id: c_int, out: *mut *mut nerf_ctx) -> c_int;
    pub fn nerf_destroy(ctx: *mut nerf_ctx);
    pub fn nerf_last_error(ctx: *const nerf_ctx) -> *const c_char;
    pub fn nerf_device_info(ctx: *const nerf_ctx, n_cus: *mut c_int, arch_name: *mut c_char, len: usize) -> c_int;
    pub fn nerf_load_network_dir(ctx: *mut nerf_ctx, which: c_int, dir: *const c_char) -> c_int;
    pub fn nerf_load_network_tensors(ctx: *mut nerf_ctx, which: c_int, n: c_int, names: *const *const c_char,
                                     dims: *const i64, data: *const *const f32) -> c_int;
    pub fn nerf_check_network_dir(dir: *const c_char) -> c_int;
    pub fn nerf_check_network_blob(blob_path: *const c_char) -> c_int;
    pub fn nerf_pack_network_dir(dir: *const c_char, blob_path: *const c_char) -> c_int;
    pub fn nerf_load_network_blob(ctx: *mut nerf_ctx, which: c_int, blob_path: *const c_char) -> c_int;
    pub fn nerf_debug_pack_network_dir(dir: *const c_char, wstream: *mut f32, wstream_cap: usize, small: *mut f32,
                                       small_cap: usize, wstream_len: *mut usize, small_len: *mut usize) -> c_int;
    pub fn nerf_debug_fold_network_dir(dir: *const c_char, wstream: *mut f32, wstream_cap: usize, small: *mut f32,
                                       small_cap: usize, wstream_len: *mut usize, small_len: *mut usize) -> c_int;
    pub fn nerf_debug_network_stream_dir(dir: *const c_char, kind: c_int, out: *mut u16, cap: usize, n: *mut usize, available: *mut c_int) -> c_int;
    pub fn nerf_debug_zero_skip_network_dir(dir: *const c_char, eligible: *mut c_int) -> c_int;
    pub fn nerf_debug_split_bf16x3(values: *const f32, n: usize, parts: *mut u16) -> c_int;
    pub fn nerf_debug_split_f16x2(values: *const f32, n: usize, parts: *mut u16) -> c_int;
    pub fn nerf_debug_certify_policy(margin: f32, audited: u64, violations: u64, headroom: f32, max_error: f32, new_margin: *mut f32) -> c_int;
    pub fn nerf_debug_ray_grouping(n_rays: c_int, samples_per_ray: c_int, enabled: c_int, first_slot_of_wave_tile: *mut i32) -> c_int;
    pub fn nerf_debug_wave_tiling(rows: c_int, rays_per_row: c_int, samples_per_ray: c_int, full: c_int, ray_grouping: c_int, wave_tiling: c_int,
                                  slot: *mut i32) -> c_int;
    pub fn nerf_debug_tile_rotation(n_tiles: c_int, n_workgroups: c_int, rotation: c_int, workgroup_of_tile: *mut i32, round_of_tile: *mut i32) -> c_int;
    pub fn nerf_debug_coarse_cut_walk(rows: c_int, rays_per_row: c_int, samples_per_ray: c_int, ray_grouping: c_int, cut_block: c_int, cut_after: c_int,
                                      tiles: *mut i32, tiles_cap: usize, blocks: *mut i32, block_tiles: *mut i32) -> c_int;
    pub fn nerf_debug_fine_cut_walk(rows: c_int, rays_per_row: c_int, samples_per_ray: c_int, cut_block: c_int, cut_after: c_int,
                                    tiles: *mut i32, tiles_cap: usize, blocks: *mut i32, block_tiles: *mut i32) -> c_int;
    pub fn nerf_debug_shader_clock_mhz(ctx: *mut nerf_ctx, mhz: *mut f64) -> c_int;
    pub fn nerf_debug_workgroup_clocks(ctx: *mut nerf_ctx, out: *mut u64, n_workgroups: usize) -> c_int;
    pub fn nerf_forward_batch(ctx: *mut nerf_ctx, which: c_int, pts_soa: *const f32, dirs_aos: *const f32, n: usize,
                              rgb_aos: *mut f32, sigma: *mut f32) -> c_int;
    pub fn nerf_forward_batch_ex(ctx: *mut nerf_ctx, which: c_int, mlp_dtype: c_int, pts_soa: *const f32, dirs_aos: *const f32,
                                 n: usize, rgb_aos: *mut f32, sigma: *mut f32) -> c_int;
    pub fn nerf_forward_batch_device(ctx: *mut nerf_ctx, which: c_int, d_pts_soa: *const f32, d_dirs_aos: *const f32,
                                     n: usize, d_rgb_aos: *mut f32, d_sigma: *mut f32, stream: *mut c_void) -> c_int;
    /// sigma alone at n points (3 x n SoA): the bits nerf_forward_batch returns as sigma, without directions or the colour head.
    pub fn nerf_density_batch(ctx: *mut nerf_ctx, which: c_int, pts_soa: *const f32, n: usize, sigma: *mut f32) -> c_int;
    pub fn nerf_density_batch_device(ctx: *mut nerf_ctx, which: c_int, d_pts_soa: *const f32, n: usize, d_sigma: *mut f32,
                                     stream: *mut c_void) -> c_int;
    /// sigma on the lattice lo + step * (ix, iy, iz) generated inside the kernel: `sigma_out` dims[2] x dims[1] x dims[0] (x fastest) or null;
    /// `occ_bits` ceil(N / 32) words (bit b of word w = sigma of cell 32 w + b > threshold) or null; `n_occupied` / `bounds` (6) optional.
    pub fn nerf_density_grid(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32, sigma_out: *mut f32,
                             threshold: f32, occ_bits: *mut u32, n_occupied: *mut u64, bounds: *mut i32) -> c_int;
    pub fn nerf_density_grid_device(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32,
                                    d_sigma_out: *mut f32, threshold: f32, d_occ_bits: *mut u32, n_occupied: *mut u64, bounds: *mut i32,
                                    stream: *mut c_void) -> c_int;
    /// The level set sigma = iso of a caller's lattice (host, dims[2] x dims[1] x dims[0], x fastest) as an indexed triangle mesh, marching
    /// tetrahedra on the device.  Arrays may be null; both counts are always returned; the arrays are written only if both counts fit the
    /// capacities (all null / 0: the size query).  Conventions: include/nerf_mi355x.h, "isosurface meshes".
    pub fn nerf_isosurface_grid(ctx: *mut nerf_ctx, sigma: *const f32, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                                vertices: *mut f32, normals: *mut f32, cap_vertices: usize, triangles: *mut u32, cap_triangles: usize,
                                n_vertices: *mut u64, n_triangles: *mut u64) -> c_int;
    /// The same on the sigma lattice of network `which`, evaluated on the device and never sent to the host; `rgb` = vertex colours.
    pub fn nerf_extract_mesh(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                             vertices: *mut f32, normals: *mut f32, rgb: *mut f32, cap_vertices: usize, triangles: *mut u32,
                             cap_triangles: usize, n_vertices: *mut u64, n_triangles: *mut u64) -> c_int;
    pub fn nerf_extract_mesh_device(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                                    d_vertices: *mut f32, d_normals: *mut f32, d_rgb: *mut f32, cap_vertices: usize, d_triangles: *mut u32,
                                    cap_triangles: usize, n_vertices: *mut u64, n_triangles: *mut u64, stream: *mut c_void) -> c_int;
    /// Connected components of the inside points (sigma > iso, 14-neighbour Kuhn connectivity) of a caller's lattice: `labels_out` N u32 or null
    /// (a component's label = its smallest linear index, 0xFFFFFFFF where not inside), `table` = `*mut nerf_component` with `cap_table` <= 64
    /// entries or null (the largest components first, ties by label), `n_components` required.
    pub fn nerf_lattice_components(ctx: *mut nerf_ctx, sigma: *const f32, dims: *const i32, iso: f32, labels_out: *mut u32, table: *mut c_void,
                                   cap_table: usize, n_components: *mut u64) -> c_int;
    /// `d_sigma` / `d_labels_out` on the device (e.g. nerf_density_grid_device's output); `table` / `n_components` on the host: synchronises `stream`.
    pub fn nerf_lattice_components_device(ctx: *mut nerf_ctx, d_sigma: *const f32, dims: *const i32, iso: f32, d_labels_out: *mut u32,
                                          table: *mut c_void, cap_table: usize, n_components: *mut u64, stream: *mut c_void) -> c_int;
    /// The mesh entry points restricted to the components `filter` (`*const nerf_component_filter` or null = everything) keeps;
    /// `n_components` / `n_kept` optional.
    pub fn nerf_isosurface_grid_filtered(ctx: *mut nerf_ctx, sigma: *const f32, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                                         filter: *const c_void, vertices: *mut f32, normals: *mut f32, cap_vertices: usize, triangles: *mut u32,
                                         cap_triangles: usize, n_vertices: *mut u64, n_triangles: *mut u64, n_components: *mut u64,
                                         n_kept: *mut u64) -> c_int;
    pub fn nerf_extract_mesh_filtered(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                                      filter: *const c_void, vertices: *mut f32, normals: *mut f32, rgb: *mut f32, cap_vertices: usize,
                                      triangles: *mut u32, cap_triangles: usize, n_vertices: *mut u64, n_triangles: *mut u64,
                                      n_components: *mut u64, n_kept: *mut u64) -> c_int;
    pub fn nerf_extract_mesh_filtered_device(ctx: *mut nerf_ctx, which: c_int, lo: *const f32, step: *const f32, dims: *const i32, iso: f32,
                                             filter: *const c_void, d_vertices: *mut f32, d_normals: *mut f32, d_rgb: *mut f32,
                                             cap_vertices: usize, d_triangles: *mut u32, cap_triangles: usize, n_vertices: *mut u64,
                                             n_triangles: *mut u64, n_components: *mut u64, n_kept: *mut u64, stream: *mut c_void) -> c_int;
    pub fn nerf_render_image(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts,
                             rgb_out: *mut f32, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_image_device(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                    d_rgb_out: *mut f32, stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// render_image + the expected-depth and opacity maps (h x w each; either may be null): include/nerf_mi355x.h defines them.
    pub fn nerf_render_image_aux(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts, rgb_out: *mut f32,
                                 depth_out: *mut f32, opacity_out: *mut f32, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_image_aux_device(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                        d_rgb_out: *mut f32, d_depth_out: *mut f32, d_opacity_out: *mut f32, stream: *mut c_void,
                                        stats: *mut nerf_stats) -> c_int;
    /// The display-ready frame, packed on the device: h x w x 4 bytes R,G,B,A (the reference's render_image_rgba, src/lib.rs:700-726).
    /// `background` null = white; `alpha_mode` = NERF_ALPHA_*.
    pub fn nerf_render_image_rgba8(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts, background: *const f32,
                                   alpha_mode: c_int, rgba_out: *mut u8, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_image_rgba8_device(ctx: *mut nerf_ctx, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                          background: *const f32, alpha_mode: c_int, d_rgba_out: *mut u8, stream: *mut c_void,
                                          stats: *mut nerf_stats) -> c_int;
    /// Render the caller's rays instead of a camera's: per-ray origins (`n_origins` = 1 or `n_rays`), directions, optional per-ray
    /// {near, far} `bounds` and RNG indices.  A batch made of a camera's rays carries the bits of `nerf_render_image_aux`.
    pub fn nerf_render_rays(ctx: *mut nerf_ctx, origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize,
                            normalize: c_int, near: f32, far: f32, bounds: *const f32, rng_index: *const u32,
                            opts: *const nerf_render_opts, background: *const f32, rgb_out: *mut f32, depth_out: *mut f32,
                            opacity_out: *mut f32, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_device(ctx: *mut nerf_ctx, d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize,
                                   normalize: c_int, near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                   opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                   d_depth_out: *mut f32, d_opacity_out: *mut f32, stream: *mut c_void,
                                   stats: *mut nerf_stats) -> c_int;
    /// `nerf_render_rays` with zero certification inside every pass (`nerf_render_opts.certify_zero` of an image render): the same bits for a
    /// fraction of the network evaluations; mlp_dtype F32, BF16X3 or F16X2.  The device form always synchronises the stream (the audit is read on the host).
    pub fn nerf_render_rays_certified(ctx: *mut nerf_ctx, origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize,
                                      normalize: c_int, near: f32, far: f32, bounds: *const f32, rng_index: *const u32,
                                      opts: *const nerf_render_opts, background: *const f32, rgb_out: *mut f32, depth_out: *mut f32,
                                      opacity_out: *mut f32, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_certified_device(ctx: *mut nerf_ctx, d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize,
                                             normalize: c_int, near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                             opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                             d_depth_out: *mut f32, d_opacity_out: *mut f32, stream: *mut c_void,
                                             stats: *mut nerf_stats) -> c_int;
    /// Central differences of sigma with step `h` at n points (3 x n SoA) -> `grad_soa` 3 x n: per axis (sigma(p + h e) - sigma(p - h e))
    /// over the f32 difference of the two coordinates, 0 where that is 0.  Conventions: include/nerf_mi355x.h, "surface normals".
    pub fn nerf_density_gradient_batch(ctx: *mut nerf_ctx, which: c_int, pts_soa: *const f32, n: usize, h: f32, grad_soa: *mut f32) -> c_int;
    pub fn nerf_density_gradient_batch_device(ctx: *mut nerf_ctx, which: c_int, d_pts_soa: *const f32, n: usize, h: f32,
                                              d_grad_soa: *mut f32, stream: *mut c_void) -> c_int;
    /// `nerf_render_rays` + one normal per ray (`normals_out` n_rays x 3): minus the weighted sum of the density gradients (step `h`) at
    /// the samples of weight > 0, normalised; zero for a ray without such a sample.  Colour, depth and opacity keep their bits.
    pub fn nerf_render_rays_normals(ctx: *mut nerf_ctx, origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize,
                                    normalize: c_int, near: f32, far: f32, bounds: *const f32, rng_index: *const u32,
                                    opts: *const nerf_render_opts, background: *const f32, rgb_out: *mut f32, depth_out: *mut f32,
                                    opacity_out: *mut f32, h: f32, normals_out: *mut f32, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_normals_device(ctx: *mut nerf_ctx, d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize,
                                           normalize: c_int, near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                           opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                           d_depth_out: *mut f32, d_opacity_out: *mut f32, h: f32, d_normals_out: *mut f32,
                                           stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// Quantile depths (include/nerf_mi355x.h, "quantile depth and point clouds"): nerf_render_rays plus `n_q` (1..8) targets in (0, 1]
    /// (`quantiles`: host memory in both forms) and one plane of n_rays depths per target (`depth_q_out`, n_q x n_rays).
    pub fn nerf_render_rays_quantiles(ctx: *mut nerf_ctx, origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize,
                                      normalize: c_int, near: f32, far: f32, bounds: *const f32, rng_index: *const u32,
                                      opts: *const nerf_render_opts, background: *const f32, rgb_out: *mut f32, depth_out: *mut f32,
                                      opacity_out: *mut f32, quantiles: *const f32, n_q: c_int, depth_q_out: *mut f32,
                                      stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_quantiles_device(ctx: *mut nerf_ctx, d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize,
                                             normalize: c_int, near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                             opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                             d_depth_out: *mut f32, d_opacity_out: *mut f32, quantiles: *const f32, n_q: c_int,
                                             d_depth_q_out: *mut f32, stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// The rays that reach `quantile` with opacity >= `min_opacity`, compacted in ray order into point records (`capacity` each; the
    /// optional arrays may be NULL, `normals_out` goes with h > 0).  NERF_ERR_STATE when more rays are kept than fit: `n_points` then
    /// carries the full count and the first `capacity` points are written.
    pub fn nerf_render_rays_points(ctx: *mut nerf_ctx, origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize,
                                   normalize: c_int, near: f32, far: f32, bounds: *const f32, rng_index: *const u32,
                                   opts: *const nerf_render_opts, quantile: f32, min_opacity: f32, h: f32, capacity: usize,
                                   xyz_out: *mut f32, rgb_out: *mut f32, normals_out: *mut f32, ray_out: *mut u32, depth_out: *mut f32,
                                   opacity_out: *mut f32, n_points: *mut usize, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_points_device(ctx: *mut nerf_ctx, d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize,
                                          normalize: c_int, near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                          opts: *const nerf_render_opts, quantile: f32, min_opacity: f32, h: f32, capacity: usize,
                                          d_xyz_out: *mut f32, d_rgb_out: *mut f32, d_normals_out: *mut f32, d_ray_out: *mut u32,
                                          d_depth_out: *mut f32, d_opacity_out: *mut f32, n_points: *mut usize, d_n_points: *mut u32,
                                          stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// Ray clipping (include/nerf_mi355x.h, "ray clipping"): grow an occupancy grid (nerf_density_grid's words) by `radius` cells (1..4,
    /// Chebyshev); `occ_bits` and `occ_out` must not overlap.  `n_occupied` / `bounds` optional, as nerf_density_grid reports them.
    pub fn nerf_occupancy_dilate(ctx: *mut nerf_ctx, occ_bits: *const u32, dims: *const i32, radius: c_int, occ_out: *mut u32,
                                 n_occupied: *mut u64, bounds: *mut i32) -> c_int;
    pub fn nerf_occupancy_dilate_device(ctx: *mut nerf_ctx, d_occ_bits: *const u32, dims: *const i32, radius: c_int, d_occ_out: *mut u32,
                                        n_occupied: *mut u64, bounds: *mut i32, stream: *mut c_void) -> c_int;
    /// Per ray the span {t_first, t_last} of the occupied cells it crosses inside its [near, far] (`bounds_out` n_rays x 2; a miss keeps
    /// its input bounds) and a 0/1 flag (`hit_out`); `n_hit` optional.  Ray arguments as nerf_render_rays.
    pub fn nerf_clip_rays(ctx: *mut nerf_ctx, occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                          origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize, normalize: c_int, near: f32, far: f32,
                          bounds: *const f32, bounds_out: *mut f32, hit_out: *mut u8, n_hit: *mut u64) -> c_int;
    pub fn nerf_clip_rays_device(ctx: *mut nerf_ctx, d_occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                                 d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize, normalize: c_int, near: f32,
                                 far: f32, d_bounds: *const f32, d_bounds_out: *mut f32, d_hit_out: *mut u8, n_hit: *mut u64,
                                 stream: *mut c_void) -> c_int;
    /// The same on the CPU, from the function the kernel calls: no context, no device.  `n_refused_reads` (optional): out-of-grid cell
    /// indices the range check turned away -- 0 unless the walk is wrong.
    pub fn nerf_debug_clip_rays(occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32, origins: *const f32,
                                n_origins: usize, dirs: *const f32, n_rays: usize, normalize: c_int, near: f32, far: f32,
                                bounds: *const f32, bounds_out: *mut f32, hit_out: *mut u8, n_hit: *mut u64,
                                n_refused_reads: *mut u64) -> c_int;
    /// Clip, drop the misses, render the rest on the device: a hit ray carries the bits of `nerf_render_rays` for that ray alone with
    /// the clipped bounds and its own rng index; a missed ray gets the background, depth 0, opacity 0.  `hit_out` / `n_hit` optional.
    pub fn nerf_render_rays_clipped(ctx: *mut nerf_ctx, occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                                    origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize, normalize: c_int, near: f32,
                                    far: f32, bounds: *const f32, rng_index: *const u32, opts: *const nerf_render_opts,
                                    background: *const f32, rgb_out: *mut f32, depth_out: *mut f32, opacity_out: *mut f32,
                                    hit_out: *mut u8, n_hit: *mut u64, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_clipped_device(ctx: *mut nerf_ctx, d_occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                                           d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize, normalize: c_int,
                                           near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                           opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                           d_depth_out: *mut f32, d_opacity_out: *mut f32, d_hit_out: *mut u8, n_hit: *mut u64,
                                           stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// `nerf_render_rays_clipped` with the compacted batch rendered under zero certification: the same bits; the device form synchronises the stream.
    pub fn nerf_render_rays_clipped_certified(ctx: *mut nerf_ctx, occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                                              origins: *const f32, n_origins: usize, dirs: *const f32, n_rays: usize, normalize: c_int, near: f32,
                                              far: f32, bounds: *const f32, rng_index: *const u32, opts: *const nerf_render_opts,
                                              background: *const f32, rgb_out: *mut f32, depth_out: *mut f32, opacity_out: *mut f32,
                                              hit_out: *mut u8, n_hit: *mut u64, stats: *mut nerf_stats) -> c_int;
    pub fn nerf_render_rays_clipped_certified_device(ctx: *mut nerf_ctx, d_occ_bits: *const u32, lo: *const f32, step: *const f32, dims: *const i32,
                                                     d_origins: *const f32, n_origins: usize, d_dirs: *const f32, n_rays: usize, normalize: c_int,
                                                     near: f32, far: f32, d_bounds: *const f32, d_rng_index: *const u32,
                                                     opts: *const nerf_render_opts, background: *const f32, d_rgb_out: *mut f32,
                                                     d_depth_out: *mut f32, d_opacity_out: *mut f32, d_hit_out: *mut u8, n_hit: *mut u64,
                                                     stream: *mut c_void, stats: *mut nerf_stats) -> c_int;
    /// render_image over several GPUs: `ctxs[i]` = one context per device, row bands on per-context host threads + streams,
    /// gathered into `rgb_out` by `gather` (NERF_GATHER_*).  The reference's counterpart is the rayon fan-out, src/lib.rs:533-557.
    pub fn nerf_render_image_multi(ctxs: *const *mut nerf_ctx, n: c_int, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                   gather: c_int, rgb_out: *mut f32, per_ctx: *mut nerf_stats) -> c_int;
    pub fn nerf_render_image_multi_aux(ctxs: *const *mut nerf_ctx, n: c_int, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                       gather: c_int, rgb_out: *mut f32, depth_out: *mut f32, opacity_out: *mut f32,
                                       per_ctx: *mut nerf_stats) -> c_int;
    pub fn nerf_render_image_multi_rgba8(ctxs: *const *mut nerf_ctx, n: c_int, cam: *const nerf_camera, opts: *const nerf_render_opts,
                                         gather: c_int, background: *const f32, alpha_mode: c_int, rgba_out: *mut u8,
                                         per_ctx: *mut nerf_stats) -> c_int;
    pub fn nerf_create_multi(device_ids: *const c_int, n: c_int, out: *mut *mut nerf_ctx) -> c_int;
    pub fn nerf_multi_release();
    pub fn nerf_band_rows(window_rows: c_int, band_index: c_int, band_count: c_int, band_stripe_rows: c_int) -> c_int;
    pub fn nerf_kernel_time_query(ctx: *mut nerf_ctx, ms: *mut f64, points: *mut u64, n_launches: *mut u32, reset: c_int) -> c_int;
    pub fn nerf_camera_from_json(json_path: *const c_char, width: c_int, height: c_int, out: *mut nerf_camera) -> c_int;
    pub fn nerf_camera_from_pose(c2w: *const f32, ref_h: f32, ref_w: f32, focal: f32, near: f32, far: f32, width: c_int,
                                 height: c_int, out: *mut nerf_camera) -> c_int;
    pub fn nerf_camera_from_values(near: f32, far: f32, origin: *const f32, forward: *const f32, up: *const f32,
                                   hwf: *const f32, width: c_int, height: c_int, out: *mut nerf_camera) -> c_int;
    pub fn nerf_save_ppm(path: *const c_char, width: c_int, height: c_int, rgb: *const f32) -> c_int;
    /// one-channel PFM ("Pf", little-endian, rows bottom-up) of a width x height map given top row first
    pub fn nerf_save_pfm(path: *const c_char, width: c_int, height: c_int, values: *const f32) -> c_int;
    /// PAM ("P7", RGB_ALPHA, MAXVAL 255) of height x width x 4 bytes
    pub fn nerf_save_pam(path: *const c_char, width: c_int, height: c_int, rgba: *const u8) -> c_int;
    /// Binary little-endian PLY of an indexed triangle mesh; `normals` / `rgb` (written as uchar) may be null.  Host-only.
    pub fn nerf_save_ply(path: *const c_char, n_vertices: usize, vertices: *const f32, normals: *const f32, rgb: *const f32,
                         n_triangles: usize, triangles: *const u32) -> c_int;
    pub fn nerf_quantize_rgb8(rgb: *const f32, n_pixels: usize, out: *mut u8);
    pub fn nerf_quantize_rgba8(rgb: *const f32, n_pixels: usize, out: *mut u8);
    pub fn nerf_stage_ray_dirs(ctx: *mut nerf_ctx, cam: *const nerf_camera, x0: c_int, y0: c_int, w: c_int, h: c_int,
                               normalize: c_int, dirs_out: *mut f32) -> c_int;
    pub fn nerf_stage_stratified(ctx: *mut nerf_ctx, cam: *const nerf_camera, x0: c_int, y0: c_int, w: c_int, h: c_int,
                                 count: c_int, seed: u64, t_out: *mut f32) -> c_int;
    pub fn nerf_stage_depth_order(ctx: *mut nerf_ctx, rows: c_int, rays_per_row: c_int, samples_per_ray: c_int, t: *const f32, table_out: *mut u32) -> c_int;
    pub fn nerf_stage_depth_order_flags(ctx: *mut nerf_ctx, rows: c_int, rays_per_row: c_int, samples_per_ray: c_int, t: *const f32, flags_out: *mut u32) -> c_int;
    pub fn nerf_stage_resample(ctx: *mut nerf_ctx, n_rays: usize, nc: c_int, nf: c_int, far: f32, seed: u64,
                               pixel_index: *const u32, t_coarse: *const f32, sigma_coarse: *const f32, u: *const f32,
                               w_out: *mut f32, cdf_out: *mut f32, t_new_out: *mut f32, t_fine_out: *mut f32) -> c_int;
    pub fn nerf_stage_hybrid_flags(ctx: *mut nerf_ctx, n_rays: usize, nc: c_int, nf: c_int, far: f32, seed: u64,
                                   pixel_index: *const u32, t_coarse: *const f32, sigma_coarse: *const f32, u: *const f32,
                                   tau: f32, flags_out: *mut u8, t_new_out: *mut f32) -> c_int;
    pub fn nerf_stage_integrate(ctx: *mut nerf_ctx, n_rays: usize, n: c_int, far: f32, rgb_aos: *const f32,
                                sigma: *const f32, t: *const f32, rgb_out: *mut f32, w_out: *mut f32) -> c_int;
    pub fn nerf_stage_integrate_rgba8(ctx: *mut nerf_ctx, n_rays: usize, n: c_int, far: f32, rgb_aos: *const f32,
                                      sigma: *const f32, t: *const f32, background: *const f32, alpha_mode: c_int,
                                      rgba_out: *mut u8) -> c_int;
    /// The quantile walk and the point compaction on caller data (one launch group each); the outputs of the second carry
    /// NERF_STAGE_GUARD_WORDS (64) guard words behind their `capacity` records.
    pub fn nerf_stage_ray_quantiles(ctx: *mut nerf_ctx, n_rays: usize, n: c_int, w: *const f32, t: *const f32, quantiles: *const f32,
                                    n_q: c_int, depth_q_out: *mut f32) -> c_int;
    pub fn nerf_stage_gather_points(ctx: *mut nerf_ctx, n_rays: usize, origins: *const f32, n_origins: usize, dirs: *const f32,
                                    depth_q: *const f32, premultiplied_rgb: *const f32, opacity: *const f32, normals: *const f32,
                                    min_opacity: f32, capacity: usize, xyz_out: *mut f32, rgb_out: *mut f32, normals_out: *mut f32,
                                    ray_out: *mut u32, depth_out: *mut f32, opacity_out: *mut f32, n_points: *mut usize) -> c_int;
    /// certify_zero's plan kernel on caller data; `list_out` / `aux_out` carry NERF_STAGE_GUARD_WORDS (64) guard words on either side
    pub fn nerf_stage_cert_plan(ctx: *mut nerf_ctx, n_rays: usize, spr: c_int, far: f32, margin: f32, depth_limit: f32, audit_mask: u32,
                                audit_mask_near: u32, audit_salt: u32, back_part: c_int, zero_threshold: f32, list_capacity: u32,
                                aux_capacity: u32, t: *const f32, pre: *mut f32, jstar_out: *mut i32, list_out: *mut u32,
                                counts_out: *mut u32, aux_out: *mut u32, rays_per_wave_out: *mut i32) -> c_int;
    pub fn nerf_stage_cert_verify(ctx: *mut nerf_ctx, n_rays: usize, spr: c_int, far: f32, list_capacity: u32, t: *const f32,
                                  jstar: *const i32, sigma: *mut f32, list_out: *mut u32, count: *mut u32,
                                  fallback_rays: *mut u32) -> c_int;
    pub fn nerf_stage_cert_audit(ctx: *mut nerf_ctx, aux: *const u32, aux_count: u32, aux_capacity: u32, n_sigma: usize,
                                 sigma: *mut f32, audit: *mut u32) -> c_int;
    pub fn nerf_stage_prefilter(ctx: *mut nerf_ctx, which: c_int, f16: c_int, origin: *const f32, dirs: *const f32, t: *const f32,
                                n_rays: usize, spr: c_int, far: f32, cut_t: f32, pre_out: *mut f32,
                                nonfinite_tiles: *mut u32) -> c_int;
    /// `nerf_stage_prefilter` with one origin per ray (`origins` n_rays x 3).
    pub fn nerf_stage_prefilter_rays(ctx: *mut nerf_ctx, which: c_int, f16: c_int, origins: *const f32, dirs: *const f32, t: *const f32,
                                     n_rays: usize, spr: c_int, far: f32, cut_t: f32, pre_out: *mut f32,
                                     nonfinite_tiles: *mut u32) -> c_int;
}

/// Compares the sizes of the `#[repr(C)]` mirrors above with the library's own structs; call once before anything else.
pub fn check_layouts() -> Result<(), String> {
    let (mut a, mut b, mut c) = (0usize, 0usize, 0usize);
    unsafe { nerf_abi_struct_sizes(&mut a, &mut b, &mut c) };
    let mine = (std::mem::size_of::<nerf_camera>(), std::mem::size_of::<nerf_render_opts>(), std::mem::size_of::<nerf_stats>());
    // the two component structs have fixed sizes (8 and 32 bytes, stated in the header)
    let components = std::mem::size_of::<nerf_component_filter>() == 8 && std::mem::size_of::<nerf_component>() == 32;
    if (a, b, c) == mine && components && unsafe { nerf_abi_version() } == 5 {
        Ok(())
    } else {
        Err(format!("libnerf_mi355x: ABI {} with struct sizes {:?}, this crate expects ABI 5 with {:?}", unsafe { nerf_abi_version() }, (a, b, c), mine))
    }
}
