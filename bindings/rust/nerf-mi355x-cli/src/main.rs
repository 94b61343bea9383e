//! The reference's `cargo run --release` (src/main.rs:1-3 -> render_cli_image, src/lib.rs:647-677) on the MI355X
//! library: same scene directory, same printed facts, same output.ppm.  Rust owns paths, camera and timing; the
//! networks live on the GPU.
use nerf_mi355x_sys as sys;
use std::ffi::{CStr, CString};
use std::path::Path;
use std::time::Instant;

fn check(ctx: *const sys::nerf_ctx, rc: i32) {
    if rc != sys::NERF_OK {
        // the reference panics in these situations (src/lib.rs:36,118,127,483-501)
        let msg = unsafe { CStr::from_ptr(sys::nerf_last_error(ctx)) }.to_string_lossy().into_owned();
        panic!("{msg}");
    }
}

fn cstr(p: &Path) -> CString {
    CString::new(p.to_str().expect("utf-8 path")).unwrap()
}

fn main() {
    let root = std::env::var("NERF_SCENE_DIR").unwrap_or_else(|_| "lego_rust".to_string());
    let root = Path::new(&root);
    sys::check_layouts().expect("libnerf_mi355x.so does not match this crate");
    let mut ctx = std::ptr::null_mut();
    check(std::ptr::null(), unsafe { sys::nerf_create(0, &mut ctx) });
    check(ctx, unsafe { sys::nerf_load_network_dir(ctx, sys::NERF_NET_COARSE, cstr(&root.join("coarse")).as_ptr()) });
    check(ctx, unsafe { sys::nerf_load_network_dir(ctx, sys::NERF_NET_FINE, cstr(&root.join("fine")).as_ptr()) });

    // beyond the reference, with the flags and meanings of nerf_cli (nerf-rs_amd/csrc/nerf_cli.cpp):
    //   --density-grid NX,NY,NZ --grid-lo X,Y,Z --grid-step SX,SY,SZ [--grid-net coarse|fine] --mesh FILE.ply [--mesh-iso V]
    //   [--mesh-keep-largest K] [--mesh-min-points M]
    // writes the sigma = V surface (default 10) of the lattice instead of rendering; K / M keep only the K largest connected components of the
    // inside points / those of at least M lattice points (nerf_extract_mesh_filtered).  The three lattice flags are required with --mesh.
    let args: Vec<String> = std::env::args().collect();
    let value = |flag: &str| args.iter().position(|a| a == flag).and_then(|i| args.get(i + 1)).cloned();
    fn triple<T: std::str::FromStr + Copy>(flag: &str, text: Option<String>) -> [T; 3] {
        let text = text.unwrap_or_else(|| panic!("--mesh needs {flag} A,B,C"));
        let v: Vec<T> = text.split(',').map(|x| x.trim().parse().unwrap_or_else(|_| panic!("{flag} A,B,C"))).collect();
        assert!(v.len() == 3, "{flag} A,B,C");
        [v[0], v[1], v[2]]
    }
    if let Some(path) = value("--mesh") {
        let iso: f32 = value("--mesh-iso").map_or(10.0, |v| v.parse().expect("--mesh-iso V"));
        let filter = sys::nerf_component_filter { keep_largest: value("--mesh-keep-largest").map_or(0, |v| v.parse().expect("--mesh-keep-largest K")),
                                                  min_points: value("--mesh-min-points").map_or(0, |v| v.parse().expect("--mesh-min-points M")) };
        let dims: [i32; 3] = triple("--density-grid", value("--density-grid"));
        let lo: [f32; 3] = triple("--grid-lo", value("--grid-lo"));
        let step: [f32; 3] = triple("--grid-step", value("--grid-step"));
        let which = match value("--grid-net").as_deref() { None | Some("fine") => sys::NERF_NET_FINE, Some("coarse") => sys::NERF_NET_COARSE,
                                                           Some(other) => panic!("--grid-net coarse|fine, not {other}") };
        let fp = &filter as *const sys::nerf_component_filter as *const std::ffi::c_void;
        let (mut nv, mut nt, mut nc, mut nk) = (0u64, 0u64, 0u64, 0u64);
        let null = std::ptr::null_mut::<f32>();
        check(ctx, unsafe {
            sys::nerf_extract_mesh_filtered(ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, fp, null, null, null, 0,
                                            std::ptr::null_mut(), 0, &mut nv, &mut nt, &mut nc, &mut nk)
        });
        let (mut v, mut n, mut t) = (vec![0f32; 3 * nv as usize], vec![0f32; 3 * nv as usize], vec![0u32; 3 * nt as usize]);
        check(ctx, unsafe {
            sys::nerf_extract_mesh_filtered(ctx, which, lo.as_ptr(), step.as_ptr(), dims.as_ptr(), iso, fp, v.as_mut_ptr(), n.as_mut_ptr(), null,
                                            nv as usize, t.as_mut_ptr(), nt as usize, &mut nv, &mut nt, std::ptr::null_mut(), std::ptr::null_mut())
        });
        check(std::ptr::null(), unsafe {
            sys::nerf_save_ply(CString::new(path).unwrap().as_ptr(), nv as usize, v.as_ptr(), n.as_ptr(), std::ptr::null(), nt as usize, t.as_ptr())
        });
        println!("mesh sigma = {iso}: {nv} vertices, {nt} triangles; {nc} components, {nk} kept");
        unsafe { sys::nerf_destroy(ctx) };
        return;
    }

    let (coarse_samples_per_ray, fine_samples_per_ray) = (64, 128); // default_sample_counts, src/lib.rs:603-612
    let (width, height) = (256, 256);                                // src/lib.rs:657-658
    println!("Rendering with {} coarse samples and {} fine samples per ray", coarse_samples_per_ray, fine_samples_per_ray);

    let mut cam = sys::nerf_camera::default();
    check(std::ptr::null(), unsafe {
        sys::nerf_camera_from_json(cstr(&root.join("tf_reference_samples.json")).as_ptr(), width, height, &mut cam)
    });
    let opts = sys::nerf_render_opts { n_coarse: coarse_samples_per_ray, n_fine: fine_samples_per_ray, ..Default::default() };

    println!("Starting image rendering...");
    let render_start = Instant::now();
    let mut image = vec![0f32; (width * height * 3) as usize];
    let mut stats = sys::nerf_stats::default();
    check(ctx, unsafe { sys::nerf_render_image(ctx, &cam, &opts, image.as_mut_ptr(), &mut stats) });
    let render_duration = render_start.elapsed();
    println!("Rendering complete: {}/{} pixels (100.0%)", width * height, width * height);
    println!("Rendering completed in {:.2} seconds", render_duration.as_secs_f64());
    println!("{:.0} rays/s on the GPU (coarse MLP {:.1} ms, fine MLP {:.1} ms, other {:.1} ms)",
             stats.n_rays as f64 / (stats.ms_total * 1e-3), stats.ms_coarse_mlp, stats.ms_fine_mlp, stats.ms_other);
    check(std::ptr::null(), unsafe { sys::nerf_save_ppm(CString::new("output.ppm").unwrap().as_ptr(), width, height, image.as_ptr()) });
    unsafe { sys::nerf_destroy(ctx) };
}
