//! Safe wrapper over `nerf-mi355x-sys`: the two seams of the reference this library replaces, with the
//! reference's own shapes --
//!   * `Gpu::forward_batch`  = `Network::forward_batch(&self, points: &Matrix /*3 x B SoA*/, view_dirs: &[Vec3])`
//!                             (reference src/network.rs:197-237)
//!   * `Gpu::render_image` / `Node::render_image` = `render_image(&coarse, &fine, &camera, fine_samples_per_ray)`
//!                             (reference src/lib.rs:474-565; `Node` = its rayon fan-out, :533-557, over the GPUs of one node)
//! Errors are `Result<_, Error>` with the library's message (the reference panics with the same text, src/lib.rs:36,118,127,
//! 483-501); contexts are freed on drop.  NOT COMPILED in the build image (no Rust toolchain there): kept small on purpose.
use nerf_mi355x_sys as sys;
use std::ffi::{CStr, CString};
use std::path::Path;

pub use sys::{nerf_camera as Camera, nerf_render_opts as RenderOpts, nerf_stats as Stats};

#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "[{}] {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}

fn check(ctx: *const sys::nerf_ctx, rc: i32) -> Result<(), Error> {
    if rc == sys::NERF_OK {
        return Ok(());
    }
    let message = unsafe { CStr::from_ptr(sys::nerf_last_error(ctx)) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

fn cpath(p: &Path) -> Result<CString, Error> {
    CString::new(p.to_string_lossy().as_bytes()).map_err(|_| Error { code: sys::NERF_ERR_INVALID, message: "path contains NUL".into() })
}

/// How `Node::render_image` brings the row bands together (include/nerf_mi355x.h, `NERF_GATHER_*`).
#[derive(Clone, Copy, Debug)]
pub enum Gather {
    Host = sys::NERF_GATHER_HOST as isize,
    Peer = sys::NERF_GATHER_PEER as isize,
    Rccl = sys::NERF_GATHER_RCCL as isize,
}

/// What the fourth byte of `Gpu::render_rgba8` holds, and what the colour bytes are relative to it (`NERF_ALPHA_*`).
#[derive(Clone, Copy, Debug)]
pub enum Alpha {
    /// colour over the background, alpha 255 (the reference's `render_image_rgba`)
    Opaque = sys::NERF_ALPHA_OPAQUE as isize,
    /// colour = sum of weight x sample colour, alpha = opacity; the background is ignored
    Premultiplied = sys::NERF_ALPHA_PREMULTIPLIED as isize,
    /// colour = premultiplied colour / opacity (0 where the opacity is 0), alpha = opacity
    Straight = sys::NERF_ALPHA_STRAIGHT as isize,
}

/// `camera_from_samples` (reference src/lib.rs:614-645) from the scene's tf_reference_samples.json.
pub fn camera_from_json(json: &Path, width: i32, height: i32) -> Result<Camera, Error> {
    let mut cam = Camera::default();
    check(std::ptr::null(), unsafe { sys::nerf_camera_from_json(cpath(json)?.as_ptr(), width, height, &mut cam) })?;
    Ok(cam)
}

/// `save_ppm` (reference src/lib.rs:567-580).
pub fn save_ppm(path: &Path, width: i32, height: i32, rgb: &[f32]) -> Result<(), Error> {
    assert_eq!(rgb.len(), (width * height * 3) as usize, "pixels.len() != width * height"); // src/lib.rs:569
    check(std::ptr::null(), unsafe { sys::nerf_save_ppm(cpath(path)?.as_ptr(), width, height, rgb.as_ptr()) })
}

/// Which connected components of the inside points a filtered mesh keeps (`nerf_component_filter`).
pub type ComponentFilter = sys::nerf_component_filter;
/// One connected component: label, number of lattice points, inclusive index bounds (`nerf_component`).
pub type Component = sys::nerf_component;

/// An indexed triangle mesh (`Gpu::extract_mesh`): `vertices`, `normals`, `colours` are V x 3, `triangles` T x 3 vertex ids.
#[derive(Debug, Clone, Default)]
pub struct Mesh {
    pub vertices: Vec<f32>,
    pub normals: Option<Vec<f32>>,
    pub colours: Option<Vec<f32>>,
    pub triangles: Vec<u32>,
}

/// What `Gpu::point_cloud` returns: one record per kept ray, in ray order (`ray`: the ray's index in the batch).
pub struct PointCloud {
    pub xyz: Vec<f32>,
    pub rgb: Vec<f32>,
    pub normals: Option<Vec<f32>>,
    pub ray: Vec<u32>,
    pub depth: Vec<f32>,
    pub opacity: Vec<f32>,
}

/// A mesh as a binary little-endian PLY (nerf_save_ply); colours are written as uchar red / green / blue.
pub fn save_ply(path: &Path, mesh: &Mesh) -> Result<(), Error> {
    let (nv, nt) = (mesh.vertices.len() / 3, mesh.triangles.len() / 3);
    let np = mesh.normals.as_ref().map_or(std::ptr::null(), |v| v.as_ptr());
    let cp = mesh.colours.as_ref().map_or(std::ptr::null(), |v| v.as_ptr());
    check(std::ptr::null(), unsafe { sys::nerf_save_ply(cpath(path)?.as_ptr(), nv, mesh.vertices.as_ptr(), np, cp, nt, mesh.triangles.as_ptr()) })
}

/// A depth or opacity map of `Gpu::render_image_aux` as a one-channel PFM (little-endian, rows bottom-up).
pub fn save_pfm(path: &Path, width: i32, height: i32, values: &[f32]) -> Result<(), Error> {
    assert_eq!(values.len(), (width * height) as usize, "values.len() != width * height");
    check(std::ptr::null(), unsafe { sys::nerf_save_pfm(cpath(path)?.as_ptr(), width, height, values.as_ptr()) })
}

/// One GPU with both networks resident (`coarse_network` / `fine_network` of render_cli_image, src/lib.rs:651-652).
pub struct Gpu {
    ctx: *mut sys::nerf_ctx,
}

// a context is single-caller but may move between threads
unsafe impl Send for Gpu {}

impl Gpu {
    /// `root` = the scene directory holding coarse/ and fine/ (`load_network_from_dir`, src/lib.rs:108-174).
    pub fn new(device: i32, root: &Path) -> Result<Self, Error> {
        sys::check_layouts().map_err(|m| Error { code: sys::NERF_ERR_STATE, message: m })?;
        let mut ctx = std::ptr::null_mut();
        check(std::ptr::null(), unsafe { sys::nerf_create(device, &mut ctx) })?;
        let gpu = Gpu { ctx }; // dropped (context destroyed) if a load below fails
        for (which, sub) in [(sys::NERF_NET_COARSE, "coarse"), (sys::NERF_NET_FINE, "fine")] {
            check(gpu.ctx, unsafe { sys::nerf_load_network_dir(gpu.ctx, which, cpath(&root.join(sub))?.as_ptr()) })?;
        }
        Ok(gpu)
    }

    /// points: 3 x B, row-major SoA (the reference's `Matrix`); view_dirs: B x 3.  Returns (colours B x 3, sigma B).
    pub fn forward_batch(&self, fine: bool, points: &[f32], view_dirs: &[f32]) -> Result<(Vec<f32>, Vec<f32>), Error> {
        assert_eq!(points.len() % 3, 0);
        let n = points.len() / 3;
        assert_eq!(view_dirs.len(), 3 * n, "one view direction per column"); // debug_assert_eq!(batch, view_dirs.len())
        let (mut rgb, mut sigma) = (vec![0f32; 3 * n], vec![0f32; n]);
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        check(self.ctx, unsafe {
            sys::nerf_forward_batch(self.ctx, which, points.as_ptr(), view_dirs.as_ptr(), n, rgb.as_mut_ptr(), sigma.as_mut_ptr())
        })?;
        Ok((rgb, sigma))
    }

    /// sigma alone at points (3 x B SoA): the bits `forward_batch` returns as sigma, without directions or the colour head.
    pub fn density(&self, fine: bool, points: &[f32]) -> Result<Vec<f32>, Error> {
        assert_eq!(points.len() % 3, 0);
        let n = points.len() / 3;
        let mut sigma = vec![0f32; n];
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        check(self.ctx, unsafe { sys::nerf_density_batch(self.ctx, which, points.as_ptr(), n, sigma.as_mut_ptr()) })?;
        Ok(sigma)
    }

    /// Central differences of sigma with step `h` (finite, > 0) at points (3 x B SoA) -> 3 x B, plane a = d sigma / d a
    /// (nerf_density_gradient_batch; the sigmas are `density`'s bits).
    pub fn density_gradient(&self, fine: bool, points: &[f32], h: f32) -> Result<Vec<f32>, Error> {
        assert_eq!(points.len() % 3, 0);
        let n = points.len() / 3;
        let mut grad = vec![0f32; 3 * n];
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        check(self.ctx, unsafe { sys::nerf_density_gradient_batch(self.ctx, which, points.as_ptr(), n, h, grad.as_mut_ptr()) })?;
        Ok(grad)
    }

    /// The density field on the lattice `lo + step * (ix, iy, iz)`, `0 <= i* < dims`, generated inside the kernel (nerf_density_grid):
    /// sigma (x fastest) if `want_sigma`, and with a `threshold` the occupancy words (bit b of word w = cell 32 w + b), the number of
    /// occupied cells and their inclusive index bounds `[ix_min, iy_min, iz_min, ix_max, iy_max, iz_max]` (none: mins = dims, maxs = -1).
    #[allow(clippy::type_complexity)]
    pub fn density_grid(&self, fine: bool, lo: [f32; 3], step: [f32; 3], dims: [i32; 3], threshold: Option<f32>, want_sigma: bool)
                        -> Result<(Option<Vec<f32>>, Option<(Vec<u32>, u64, [i32; 6])>), Error> {
        let n = dims.iter().map(|&d| d.max(0) as usize).product::<usize>(); // a dim <= 0: the library refuses the call
        let mut sigma = if want_sigma { Some(vec![0f32; n]) } else { None };
        let mut occ = threshold.map(|_| (vec![0u32; (n + 31) / 32], 0u64, [0i32; 6]));
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        let sp = sigma.as_mut().map_or(std::ptr::null_mut(), |v| v.as_mut_ptr());
        let (bp, cp, rp) = occ.as_mut().map_or((std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()),
                                               |o| (o.0.as_mut_ptr(), &mut o.1 as *mut u64, o.2.as_mut_ptr()));
        check(self.ctx, unsafe {
            sys::nerf_density_grid(self.ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), sp, threshold.unwrap_or(0.0), bp, cp, rp)
        })?;
        Ok((sigma, occ))
    }

    /// The level set sigma = `iso` of a network on the lattice of `density_grid` (every dim >= 2, no zero step) as a welded, indexed
    /// triangle mesh, extracted on the device by marching tetrahedra (nerf_extract_mesh; conventions in include/nerf_mi355x.h).  The
    /// sigma lattice never reaches the host.  A size query is followed by the fill: the lattice is evaluated twice.
    pub fn extract_mesh(&self, fine: bool, lo: [f32; 3], step: [f32; 3], dims: [i32; 3], iso: f32, normals: bool, colours: bool) -> Result<Mesh, Error> {
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        let (mut nv, mut nt) = (0u64, 0u64);
        let null = std::ptr::null_mut::<f32>();
        check(self.ctx, unsafe {
            sys::nerf_extract_mesh(self.ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, null, null, null, 0, std::ptr::null_mut(), 0, &mut nv, &mut nt)
        })?;
        let (cap_v, cap_t) = (nv as usize, nt as usize);
        let mut mesh = Mesh { vertices: vec![0f32; 3 * cap_v], normals: if normals { Some(vec![0f32; 3 * cap_v]) } else { None },
                              colours: if colours { Some(vec![0f32; 3 * cap_v]) } else { None }, triangles: vec![0u32; 3 * cap_t] };
        let np = mesh.normals.as_mut().map_or(null, |v| v.as_mut_ptr());
        let cp = mesh.colours.as_mut().map_or(null, |v| v.as_mut_ptr());
        check(self.ctx, unsafe {
            sys::nerf_extract_mesh(self.ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, mesh.vertices.as_mut_ptr(), np, cp, cap_v,
                                   mesh.triangles.as_mut_ptr(), cap_t, &mut nv, &mut nt)
        })?;
        assert!(nv as usize == cap_v && nt as usize == cap_t, "the mesh changed between the size query and the fill");
        Ok(mesh)
    }

    /// The same for a caller's sigma lattice (`sigma.len() == dims[0] * dims[1] * dims[2]`, x fastest): nerf_isosurface_grid; no network needed.
    pub fn isosurface(&self, sigma: &[f32], lo: [f32; 3], step: [f32; 3], dims: [i32; 3], iso: f32, normals: bool) -> Result<Mesh, Error> {
        assert_eq!(sigma.len(), dims.iter().map(|&d| d.max(0) as usize).product::<usize>(), "one sigma per lattice point");
        let (mut nv, mut nt) = (0u64, 0u64);
        let null = std::ptr::null_mut::<f32>();
        check(self.ctx, unsafe {
            sys::nerf_isosurface_grid(self.ctx, sigma.as_ptr(), lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, null, null, 0, std::ptr::null_mut(), 0, &mut nv, &mut nt)
        })?;
        let (cap_v, cap_t) = (nv as usize, nt as usize);
        let mut mesh = Mesh { vertices: vec![0f32; 3 * cap_v], normals: if normals { Some(vec![0f32; 3 * cap_v]) } else { None }, colours: None,
                              triangles: vec![0u32; 3 * cap_t] };
        let np = mesh.normals.as_mut().map_or(null, |v| v.as_mut_ptr());
        check(self.ctx, unsafe {
            sys::nerf_isosurface_grid(self.ctx, sigma.as_ptr(), lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, mesh.vertices.as_mut_ptr(), np, cap_v,
                                      mesh.triangles.as_mut_ptr(), cap_t, &mut nv, &mut nt)
        })?;
        Ok(mesh)
    }

    /// `extract_mesh` restricted to the components `filter` keeps (nerf_extract_mesh_filtered; "lattice components" in the header): the
    /// inside points (sigma > iso) are split into connected pieces under the 14-neighbour Kuhn connectivity, ranked by size (ties: smaller
    /// label first); `keep_largest: 1` drops every floater.  Returns the mesh, the number of components and the number kept.
    pub fn extract_mesh_filtered(&self, fine: bool, lo: [f32; 3], step: [f32; 3], dims: [i32; 3], iso: f32, filter: ComponentFilter, normals: bool,
                                 colours: bool) -> Result<(Mesh, u64, u64), Error> {
        let which = if fine { sys::NERF_NET_FINE } else { sys::NERF_NET_COARSE };
        let (mut nv, mut nt, mut nc, mut nk) = (0u64, 0u64, 0u64, 0u64);
        let null = std::ptr::null_mut::<f32>();
        let fp = &filter as *const ComponentFilter as *const std::ffi::c_void;
        check(self.ctx, unsafe {
            sys::nerf_extract_mesh_filtered(self.ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, fp, null, null, null, 0, std::ptr::null_mut(), 0,
                                            &mut nv, &mut nt, &mut nc, &mut nk)
        })?;
        let (cap_v, cap_t) = (nv as usize, nt as usize);
        let mut mesh = Mesh { vertices: vec![0f32; 3 * cap_v], normals: if normals { Some(vec![0f32; 3 * cap_v]) } else { None },
                              colours: if colours { Some(vec![0f32; 3 * cap_v]) } else { None }, triangles: vec![0u32; 3 * cap_t] };
        let np = mesh.normals.as_mut().map_or(null, |v| v.as_mut_ptr());
        let cp = mesh.colours.as_mut().map_or(null, |v| v.as_mut_ptr());
        check(self.ctx, unsafe {
            sys::nerf_extract_mesh_filtered(self.ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, fp, mesh.vertices.as_mut_ptr(), np, cp, cap_v,
                                            mesh.triangles.as_mut_ptr(), cap_t, &mut nv, &mut nt, std::ptr::null_mut(), std::ptr::null_mut())
        })?;
        assert!(nv as usize == cap_v && nt as usize == cap_t, "the mesh changed between the size query and the fill");
        Ok((mesh, nc, nk))
    }

    /// The connected components of the inside points of a caller's sigma lattice (nerf_lattice_components): per point its component's label
    /// (the smallest linear index of the component; 0xFFFFFFFF where not inside), the `table` (<= 64) largest components in rank order, and
    /// the number of components.
    pub fn lattice_components(&self, sigma: &[f32], dims: [i32; 3], iso: f32, table: usize) -> Result<(Vec<u32>, Vec<Component>, u64), Error> {
        assert_eq!(sigma.len(), dims.iter().map(|&d| d.max(0) as usize).product::<usize>(), "one sigma per lattice point");
        let mut labels = vec![0u32; sigma.len()];
        let mut entries = vec![Component::default(); table];
        let mut n = 0u64;
        let tp = if table > 0 { entries.as_mut_ptr() as *mut std::ffi::c_void } else { std::ptr::null_mut() };
        check(self.ctx, unsafe { sys::nerf_lattice_components(self.ctx, sigma.as_ptr(), dims.as_ptr(), iso, labels.as_mut_ptr(), tp, table, &mut n) })?;
        entries.truncate((n as usize).min(table));
        Ok((labels, entries, n))
    }

    /// Linear RGB, pixel (i, j) at `(i * w + j) * 3` (image[i * nx + j], src/lib.rs:552-557); `opts.n_coarse` = camera.samples_per_ray.
    pub fn render_image(&self, cam: &Camera, opts: &RenderOpts) -> Result<(Vec<f32>, Stats), Error> {
        let (w, h) = if opts.crop_w > 0 || opts.crop_h > 0 { (opts.crop_w, opts.crop_h) } else { (cam.nx, cam.ny) };
        let mut image = vec![0f32; (w.max(0) as usize) * (h.max(0) as usize) * 3];
        let mut stats = Stats::default();
        check(self.ctx, unsafe { sys::nerf_render_image(self.ctx, cam, opts, image.as_mut_ptr(), &mut stats) })?;
        Ok((image, stats))
    }

    /// `render_image` plus the expected-depth map (distance along the unit ray, 0 for the background) and the opacity map
    /// (accumulated weight), one f32 per pixel each in the same pixel order (nerf_render_image_aux).
    pub fn render_image_aux(&self, cam: &Camera, opts: &RenderOpts) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>, Stats), Error> {
        let (w, h) = if opts.crop_w > 0 || opts.crop_h > 0 { (opts.crop_w, opts.crop_h) } else { (cam.nx, cam.ny) };
        let px = (w.max(0) as usize) * (h.max(0) as usize);
        let (mut image, mut depth, mut opacity) = (vec![0f32; px * 3], vec![0f32; px], vec![0f32; px]);
        let mut stats = Stats::default();
        check(self.ctx, unsafe {
            sys::nerf_render_image_aux(self.ctx, cam, opts, image.as_mut_ptr(), depth.as_mut_ptr(), opacity.as_mut_ptr(), &mut stats)
        })?;
        Ok((image, depth, opacity, stats))
    }

    /// The display-ready frame, packed on the device: R,G,B,A bytes, pixel (i, j) at `(i * w + j) * 4` (the reference's
    /// `render_image_rgba`, src/lib.rs:700-726, is `render_rgba8(cam, opts, None, Alpha::Opaque)`).  `background` None = white.
    pub fn render_rgba8(&self, cam: &Camera, opts: &RenderOpts, background: Option<[f32; 3]>, alpha: Alpha) -> Result<(Vec<u8>, Stats), Error> {
        let (w, h) = if opts.crop_w > 0 || opts.crop_h > 0 { (opts.crop_w, opts.crop_h) } else { (cam.nx, cam.ny) };
        let mut rgba = vec![0u8; (w.max(0) as usize) * (h.max(0) as usize) * 4];
        let mut stats = Stats::default();
        let bg = background.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        check(self.ctx, unsafe { sys::nerf_render_image_rgba8(self.ctx, cam, opts, bg, alpha as i32, rgba.as_mut_ptr(), &mut stats) })?;
        Ok((rgba, stats))
    }

    /// The caller's rays instead of a camera's (nerf_render_rays): `origins` holds one origin (3 floats) for every ray or one per ray,
    /// `dirs` n x 3 (normalised on the device when `normalize`), `bounds` optional n x 2 {near, far} (else `near`, `far` for every ray),
    /// `rng_index` optional n (else ray r draws from index r).  `opts` as for an image, without the pixel-grid and skip options.
    /// -> (rgb n x 3, depth n, opacity n, stats).
    #[allow(clippy::too_many_arguments)]
    pub fn render_rays(&self, origins: &[f32], dirs: &[f32], normalize: bool, near: f32, far: f32, bounds: Option<&[f32]>,
                       rng_index: Option<&[u32]>, opts: &RenderOpts, background: Option<[f32; 3]>) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>, Stats), Error> {
        let n = dirs.len() / 3;
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        assert!(rng_index.map_or(true, |i| i.len() == n), "rng_index.len() must be n_rays");
        let (mut rgb, mut depth, mut opacity) = (vec![0f32; 3 * n], vec![0f32; n], vec![0f32; n]);
        let mut stats = Stats::default();
        let bg = background.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        check(self.ctx, unsafe {
            sys::nerf_render_rays(self.ctx, origins.as_ptr(), origins.len() / 3, dirs.as_ptr(), n, normalize as i32, near, far,
                                  bounds.map_or(std::ptr::null(), |b| b.as_ptr()), rng_index.map_or(std::ptr::null(), |i| i.as_ptr()), opts, bg,
                                  rgb.as_mut_ptr(), depth.as_mut_ptr(), opacity.as_mut_ptr(), &mut stats)
        })?;
        Ok((rgb, depth, opacity, stats))
    }

    /// `render_rays` with zero certification inside every pass (nerf_render_rays_certified; `RenderOpts.certify_zero` of an image render): the
    /// same bits for a fraction of the network evaluations; `stats` carries the audit.  mlp_dtype F32, BF16X3 or F16X2.
    #[allow(clippy::too_many_arguments)]
    pub fn render_rays_certified(&self, origins: &[f32], dirs: &[f32], normalize: bool, near: f32, far: f32, bounds: Option<&[f32]>,
                                 rng_index: Option<&[u32]>, opts: &RenderOpts, background: Option<[f32; 3]>) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>, Stats), Error> {
        let n = dirs.len() / 3;
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        assert!(rng_index.map_or(true, |i| i.len() == n), "rng_index.len() must be n_rays");
        let (mut rgb, mut depth, mut opacity) = (vec![0f32; 3 * n], vec![0f32; n], vec![0f32; n]);
        let mut stats = Stats::default();
        let bg = background.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        check(self.ctx, unsafe {
            sys::nerf_render_rays_certified(self.ctx, origins.as_ptr(), origins.len() / 3, dirs.as_ptr(), n, normalize as i32, near, far,
                                            bounds.map_or(std::ptr::null(), |b| b.as_ptr()), rng_index.map_or(std::ptr::null(), |i| i.as_ptr()), opts, bg,
                                            rgb.as_mut_ptr(), depth.as_mut_ptr(), opacity.as_mut_ptr(), &mut stats)
        })?;
        Ok((rgb, depth, opacity, stats))
    }

    /// `render_rays` with one normal per ray (nerf_render_rays_normals): minus the weighted sum of the density gradients, step `h`, at
    /// the samples of weight > 0, normalised; (0, 0, 0) for a ray without such a sample.  -> (rgb, depth, opacity, normals n x 3, stats);
    /// the first three are `render_rays`' bits.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn render_rays_normals(&self, origins: &[f32], dirs: &[f32], normalize: bool, near: f32, far: f32, bounds: Option<&[f32]>,
                               rng_index: Option<&[u32]>, opts: &RenderOpts, background: Option<[f32; 3]>, h: f32)
                               -> Result<(Vec<f32>, Vec<f32>, Vec<f32>, Vec<f32>, Stats), Error> {
        let n = dirs.len() / 3;
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        assert!(rng_index.map_or(true, |i| i.len() == n), "rng_index.len() must be n_rays");
        let (mut rgb, mut depth, mut opacity, mut normals) = (vec![0f32; 3 * n], vec![0f32; n], vec![0f32; n], vec![0f32; 3 * n]);
        let mut stats = Stats::default();
        let bg = background.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        check(self.ctx, unsafe {
            sys::nerf_render_rays_normals(self.ctx, origins.as_ptr(), origins.len() / 3, dirs.as_ptr(), n, normalize as i32, near, far,
                                          bounds.map_or(std::ptr::null(), |b| b.as_ptr()), rng_index.map_or(std::ptr::null(), |i| i.as_ptr()), opts,
                                          bg, rgb.as_mut_ptr(), depth.as_mut_ptr(), opacity.as_mut_ptr(), h, normals.as_mut_ptr(), &mut stats)
        })?;
        Ok((rgb, depth, opacity, normals, stats))
    }

    /// The coloured point cloud of a ray batch (nerf_render_rays_points): one point per ray whose running sum of compositing weights
    /// reaches `quantile` (0.5: the median depth) with opacity >= `min_opacity`, in ray order.  `h`: central-difference step of the
    /// normals, or None for a cloud without them.  The ray arguments are `render_rays`'.
    #[allow(clippy::too_many_arguments)]
    pub fn point_cloud(&self, origins: &[f32], dirs: &[f32], normalize: bool, near: f32, far: f32, bounds: Option<&[f32]>,
                       rng_index: Option<&[u32]>, opts: &RenderOpts, quantile: f32, min_opacity: f32, h: Option<f32>)
                       -> Result<PointCloud, Error> {
        let n = dirs.len() / 3;
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        assert!(rng_index.map_or(true, |i| i.len() == n), "rng_index.len() must be n_rays");
        let (mut xyz, mut rgb, mut depth, mut opacity, mut ray) = (vec![0f32; 3 * n], vec![0f32; 3 * n], vec![0f32; n], vec![0f32; n], vec![0u32; n]);
        let mut normals = h.map(|_| vec![0f32; 3 * n]);
        let mut kept = 0usize;
        check(self.ctx, unsafe {
            sys::nerf_render_rays_points(self.ctx, origins.as_ptr(), origins.len() / 3, dirs.as_ptr(), n, normalize as i32, near, far,
                                         bounds.map_or(std::ptr::null(), |b| b.as_ptr()), rng_index.map_or(std::ptr::null(), |i| i.as_ptr()), opts,
                                         quantile, min_opacity, h.unwrap_or(0.0), n, xyz.as_mut_ptr(), rgb.as_mut_ptr(),
                                         normals.as_mut().map_or(std::ptr::null_mut(), |v| v.as_mut_ptr()), ray.as_mut_ptr(), depth.as_mut_ptr(),
                                         opacity.as_mut_ptr(), &mut kept, std::ptr::null_mut())
        })?;
        xyz.truncate(3 * kept); rgb.truncate(3 * kept); depth.truncate(kept); opacity.truncate(kept); ray.truncate(kept);
        if let Some(v) = normals.as_mut() { v.truncate(3 * kept); }
        Ok(PointCloud { xyz, rgb, normals, ray, depth, opacity })
    }

    /// Grow the occupancy words of `density_grid` by `radius` cells (1..4, Chebyshev distance; nerf_occupancy_dilate)
    /// -> (words, occupied cells, inclusive index bounds).
    pub fn dilate_occupancy(&self, bits: &[u32], dims: [i32; 3], radius: i32) -> Result<(Vec<u32>, u64, [i32; 6]), Error> {
        let n = dims.iter().map(|&d| d.max(0) as usize).product::<usize>(); // a dim <= 0: the library refuses the call
        assert!(n == 0 || bits.len() == (n + 31) / 32, "bits.len() must be ceil(n_cells / 32)");
        let (mut out, mut count, mut bounds) = (vec![0u32; bits.len()], 0u64, [0i32; 6]);
        check(self.ctx, unsafe {
            sys::nerf_occupancy_dilate(self.ctx, bits.as_ptr(), dims.as_ptr(), radius, out.as_mut_ptr(), &mut count, bounds.as_mut_ptr())
        })?;
        Ok((out, count, bounds))
    }

    /// Per ray the span of the occupied cells of an occupancy grid (words over the lattice `lo`, `step`, `dims`) inside the ray's
    /// [near, far] (nerf_clip_rays; ray arguments as `render_rays`) -> (bounds n x 2, hit flags n, number of hits): a hit ray's
    /// bounds are {t_first, t_last}, ready for `render_rays`; a missed ray keeps its input {near, far}.
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn clip_rays(&self, bits: &[u32], lo: [f32; 3], step: [f32; 3], dims: [i32; 3], origins: &[f32], dirs: &[f32], normalize: bool,
                     near: f32, far: f32, bounds: Option<&[f32]>) -> Result<(Vec<f32>, Vec<u8>, u64), Error> {
        let n = dirs.len() / 3;
        let cells = dims.iter().map(|&d| d.max(0) as usize).product::<usize>();
        assert!(cells == 0 || bits.len() == (cells + 31) / 32, "bits.len() must be ceil(n_cells / 32)");
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        let (mut out, mut hit, mut n_hit) = (vec![0f32; 2 * n], vec![0u8; n], 0u64);
        check(self.ctx, unsafe {
            sys::nerf_clip_rays(self.ctx, bits.as_ptr(), lo.as_ptr(), step.as_ptr(), dims.as_ptr(), origins.as_ptr(), origins.len() / 3, dirs.as_ptr(), n,
                                normalize as i32, near, far, bounds.map_or(std::ptr::null(), |b| b.as_ptr()), out.as_mut_ptr(), hit.as_mut_ptr(),
                                &mut n_hit)
        })?;
        Ok((out, hit, n_hit))
    }

    /// `render_rays` behind `clip_rays`, on the device (nerf_render_rays_clipped): the rays that cross an occupied cell are rendered
    /// over their clipped bounds -- `render_rays`' bits for those rays alone --, the others get the background, depth 0 and opacity 0.
    /// -> (rgb n x 3, depth n, opacity n, hit flags n, number of hits, stats of the compacted batch).
    #[allow(clippy::too_many_arguments, clippy::type_complexity)]
    pub fn render_rays_clipped(&self, bits: &[u32], lo: [f32; 3], step: [f32; 3], dims: [i32; 3], origins: &[f32], dirs: &[f32], normalize: bool,
                               near: f32, far: f32, bounds: Option<&[f32]>, rng_index: Option<&[u32]>, opts: &RenderOpts,
                               background: Option<[f32; 3]>) -> Result<(Vec<f32>, Vec<f32>, Vec<f32>, Vec<u8>, u64, Stats), Error> {
        let n = dirs.len() / 3;
        let cells = dims.iter().map(|&d| d.max(0) as usize).product::<usize>();
        assert!(cells == 0 || bits.len() == (cells + 31) / 32, "bits.len() must be ceil(n_cells / 32)");
        assert_eq!(dirs.len(), 3 * n, "dirs.len() must be 3 * n_rays");
        assert!(origins.len() == 3 || origins.len() == 3 * n, "origins must hold one origin or one per ray");
        assert!(bounds.map_or(true, |b| b.len() == 2 * n), "bounds.len() must be 2 * n_rays");
        assert!(rng_index.map_or(true, |i| i.len() == n), "rng_index.len() must be n_rays");
        let (mut rgb, mut depth, mut opacity, mut hit, mut n_hit) = (vec![0f32; 3 * n], vec![0f32; n], vec![0f32; n], vec![0u8; n], 0u64);
        let mut stats = Stats::default();
        let bg = background.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        check(self.ctx, unsafe {
            sys::nerf_render_rays_clipped(self.ctx, bits.as_ptr(), lo.as_ptr(), step.as_ptr(), dims.as_ptr(), origins.as_ptr(), origins.len() / 3,
                                          dirs.as_ptr(), n, normalize as i32, near, far, bounds.map_or(std::ptr::null(), |b| b.as_ptr()),
                                          rng_index.map_or(std::ptr::null(), |i| i.as_ptr()), opts, bg, rgb.as_mut_ptr(), depth.as_mut_ptr(),
                                          opacity.as_mut_ptr(), hit.as_mut_ptr(), &mut n_hit, &mut stats)
        })?;
        Ok((rgb, depth, opacity, hit, n_hit, stats))
    }
}

impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { sys::nerf_destroy(self.ctx) }
    }
}

/// All GPUs of one node: one context per device, weights replicated, row bands gathered into one image.
pub struct Node {
    gpus: Vec<Gpu>,
}

impl Node {
    pub fn new(devices: &[i32], root: &Path) -> Result<Self, Error> {
        Ok(Node { gpus: devices.iter().map(|&d| Gpu::new(d, root)).collect::<Result<_, _>>()? })
    }

    pub fn render_image(&self, cam: &Camera, opts: &RenderOpts, gather: Gather) -> Result<(Vec<f32>, Vec<Stats>), Error> {
        let (w, h) = if opts.crop_w > 0 || opts.crop_h > 0 { (opts.crop_w, opts.crop_h) } else { (cam.nx, cam.ny) };
        let mut image = vec![0f32; (w.max(0) as usize) * (h.max(0) as usize) * 3];
        let mut stats = vec![Stats::default(); self.gpus.len()];
        let ctxs: Vec<*mut sys::nerf_ctx> = self.gpus.iter().map(|g| g.ctx).collect();
        let first = ctxs.first().copied().unwrap_or(std::ptr::null_mut());
        check(first, unsafe {
            sys::nerf_render_image_multi(ctxs.as_ptr(), ctxs.len() as i32, cam, opts, gather as i32, image.as_mut_ptr(), stats.as_mut_ptr())
        })?;
        Ok((image, stats))
    }
}
