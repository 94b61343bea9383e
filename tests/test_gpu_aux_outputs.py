"""Expected-depth and opacity maps (nerf_render_image_aux, nerf_render_image_multi_aux): against the CPU oracle, bit-identical
colour in every mode, maps that follow the exact modes bit for bit, multi-GPU gathers, SSAA, whole-frame invariants and the CLI.

Definitions (include/nerf_mi355x.h): opacity = sum_i w_i, depth = sum_i (t_i * w_i), both in sample order in f32, with w_i the exact
compositing weights (zero after the T < 1e-4 cut) and t_i the ray's own sample positions."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE, golden

pytestmark = pytest.mark.gpu

FIX = "aux_c3_800.npz"


def _gate(got, want, far=1.0):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert d.max() <= 5e-4 * far and d.mean() <= 1e-5 * far, (d.max(), d.mean())
    return d


def _seq_maps(w, t):
    """The oracle's sums: sample order, f32, separate multiply and add."""
    dep = np.float32(0.0); acc = np.float32(0.0)
    for i in range(len(w)):
        dep = np.float32(dep + np.float32(t[i] * w[i]))
        acc = np.float32(acc + w[i])
    return dep, acc


@pytest.fixture(scope="module")
def cam800(native, samples):
    return native.camera_from_samples(samples, 800, 800, 64)


def _aux(native, r, cam, nf=128, **kw):
    return native.render_image(r.coarse, r.fine, cam, nf, aux=True, **kw)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["centre", "silhouette"])
def test_maps_match_oracle_crops(native, renderer, cam800, name):
    g = golden(FIX)
    far = float(g["far"])
    crop = tuple(int(v) for v in g[f"{name}_crop"])
    rgb, depth, opacity = _aux(native, renderer, cam800, seed=0, crop=crop)
    do = _gate(opacity, g[f"{name}_opacity"])
    dd = _gate(depth, g[f"{name}_depth"], far)
    dc = np.abs(rgb - g[f"{name}_rgb"])
    assert dc.max() <= 5e-4 and dc.mean() <= 1e-5
    print(f"{name}: opacity max {do.max():.3e} mean {do.mean():.3e}; depth max {dd.max():.3e} mean {dd.mean():.3e} (far {far})")


# ---- 2. the 32 stage-fixture rays ---------------------------------------------------------------------------------------------
def test_stage_fixture_rays(native, renderer, cam800):
    st = golden("ray_stages_800.npz")
    far = float(st["far"])
    got_d, got_o, want_d, want_o = [], [], [], []
    for k, (i, j) in enumerate(st["pixels"]):
        _, d, o = _aux(native, renderer, cam800, seed=int(st["seed"]), crop=(int(j), int(i), 1, 1))
        wd, wo = _seq_maps(st["w_fine"][k], st["t_merged"][k])
        got_d.append(d[0, 0]); got_o.append(o[0, 0]); want_d.append(wd); want_o.append(wo)
        if st["is_empty"][k]:
            assert d[0, 0] == 0.0 and o[0, 0] == 0.0                   # an empty ray: depth 0, opacity 0
        if st["is_terminated"][k]:
            assert o[0, 0] > 0.999                                        # cut at T < 1e-4: opacity above 1 - 1e-4 up to rounding
    _gate(np.array(got_o), np.array(want_o))
    _gate(np.array(got_d), np.array(want_d), far)
    assert st["is_empty"].any() and st["is_terminated"].any()


# ---- 3. colour unchanged, 4. maps follow the exact modes ----------------------------------------------------------------------
MODES = {
    "f32": {}, "bf16": dict(dtype="bf16"), "bf16x3": dict(dtype="bf16x3"), "f16x2": dict(dtype="f16x2"),
    "skip_empty": dict(skip_empty=True), "skip_dead": dict(skip_dead=True), "certify_zero": dict(certify_zero=True),
    "hybrid_sampling": dict(skip_dead=True, hybrid_sampling=True), "coarse_only": dict(coarse_only=True), "n_fine0": dict(nf=0),
    "ssaa2": dict(ssaa=2), "ragged": dict(crop=(311, 287, 53, 29)),
    "band_contiguous": dict(band=(1, 3, 0)), "band_striped": dict(band=(2, 3, 1)),
}
WINDOW = (300, 330, 96, 40)


@pytest.mark.parametrize("mode", list(MODES))
def test_colour_is_bit_identical_with_maps(native, renderer, cam800, mode):
    kw = dict(MODES[mode])
    nf = kw.pop("nf", 128)
    kw.setdefault("crop", WINDOW)
    plain = native.render_image(renderer.coarse, renderer.fine, cam800, nf, seed=0, **kw)
    rgb, depth, opacity = _aux(native, renderer, cam800, nf, seed=0, **kw)
    assert np.array_equal(rgb, plain)
    assert depth.shape == opacity.shape == plain.shape[:2]
    assert np.isfinite(depth).all() and np.isfinite(opacity).all()
    if "band" in kw:  # a band's maps are the same rows of the whole window's maps, bit for bit
        whole = _aux(native, renderer, cam800, nf, seed=0, **{k: v for k, v in kw.items() if k != "band"})
        rows = native.band_row_indices(kw["crop"][3], *kw["band"])
        for a, b in zip((rgb, depth, opacity), whole):
            assert np.array_equal(a, b[rows])


def test_maps_follow_the_exact_modes(native, renderer, cam800):
    crop = (280, 300, 128, 64)
    ref = _aux(native, renderer, cam800, seed=0, crop=crop)
    for kw in (dict(skip_empty=True), dict(skip_dead=True), dict(certify_zero=True)):
        got = _aux(native, renderer, cam800, seed=0, crop=crop, **kw)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), kw
    ref16 = _aux(native, renderer, cam800, seed=0, crop=crop, dtype="f16x2")
    cert16 = _aux(native, renderer, cam800, seed=0, crop=crop, dtype="f16x2", certify_zero=True)
    for a, b in zip(cert16, ref16):
        assert np.array_equal(a, b)
    assert (ref[2] > 0.99).mean() > 0.2 and (ref[2] < 0.01).mean() > 0.05   # the window holds both model and background


def test_one_map_at_a_time_and_device_entry_point(native, renderer, cam800):
    """Either map may be NULL; the device entry point (device buffers from the HIP runtime) writes the same bits as the host one."""
    import ctypes as C
    from nerf_rs_amd import _lib
    crop = (350, 380, 33, 17)
    rgb, depth, opacity = _aux(native, renderer, cam800, seed=0, crop=crop)
    L = native.load_library()
    opts = native.RenderOpts(64, 128, False, crop, 1, 0, "f32", False, False, False, False, None).to_c()
    for want_d, want_o in ((True, False), (False, True)):
        out = np.empty_like(rgb); d = np.full(depth.shape, -7, np.float32); o = np.full(depth.shape, -7, np.float32)
        rc = L.nerf_render_image_aux(renderer.handle, C.byref(cam800.c), C.byref(opts), out.ctypes.data_as(_lib.f32p),
                                     d.ctypes.data_as(_lib.f32p) if want_d else None, o.ctypes.data_as(_lib.f32p) if want_o else None, None)
        assert rc == 0 and np.array_equal(out, rgb)
        assert np.array_equal(d, depth) if want_d else (d == -7).all()
        assert np.array_equal(o, opacity) if want_o else (o == -7).all()
    hip = C.CDLL("libamdhip64.so.7")                # the runtime the library itself links (already loaded)
    bufs = [C.c_void_p() for _ in range(3)]
    sizes = (rgb.nbytes, depth.nbytes, opacity.nbytes)
    for b, n in zip(bufs, sizes):
        assert hip.hipMalloc(C.byref(b), C.c_size_t(n)) == 0
    try:
        native.render_image(renderer.coarse, renderer.fine, cam800, 128, seed=0, crop=crop, aux=True, device_out=bufs[0].value,
                            device_depth=bufs[1].value, device_opacity=bufs[2].value, return_stats=True)   # stats: synchronises
        for b, n, want in zip(bufs, sizes, (rgb, depth, opacity)):
            got = np.empty_like(want)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), b, C.c_size_t(n), 2) == 0   # hipMemcpyDeviceToHost
            assert np.array_equal(got, want)
    finally:
        for b in bufs:
            hip.hipFree(b)
    assert L.nerf_render_image_aux(renderer.handle, C.byref(cam800.c), C.byref(opts), None, d.ctypes.data_as(_lib.f32p), None, None) == -1


# ---- 5. multi-GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(native):
    rs = [native.Renderer(0) for _ in range(3)]
    for r in rs:
        r.load_scene(SCENE)
    yield rs
    for r in rs:
        r.close()


@pytest.mark.parametrize("striped", [False, True], ids=["contiguous", "striped"])
@pytest.mark.parametrize("gather", ["host", "peer", "rccl"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_multi_aux_is_bit_identical_to_one_context(native, renderer, cam800, three, n, gather, striped):
    crop = (200, 300, 400, 101)                       # 101 rows: ragged over 2 and 3 bands
    kw = dict(seed=0, crop=crop, skip_dead=striped)   # skip_dead: rows dealt out round-robin
    ref = _aux(native, renderer, cam800, **kw)
    got = native.render_image_multi(three[:n], cam800, 128, gather=gather, aux=True, **kw)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    plain = native.render_image_multi(three[:n], cam800, 128, gather=gather, **kw)
    assert np.array_equal(plain, ref[0])              # and the colour-only call is unchanged


# ---- 6. whole-frame invariants -------------------------------------------------------------------------------------------------
def test_full_frame_invariants(native, renderer, cam800):
    rgb, depth, opacity = _aux(native, renderer, cam800, seed=0)
    far = np.float32(cam800.far)
    assert np.isfinite(depth).all() and np.isfinite(opacity).all()
    assert opacity.min() >= 0.0 and opacity.max() <= 1 + 1e-6
    assert depth.min() >= 0.0 and (depth <= far * opacity * np.float32(1 + 1e-6)).all()
    # background: the top rows (no model there).  A white pixel elsewhere is not necessarily background: colours are sigmoids that
    # saturate to exactly 1.0, and the oracle's silhouette crop has white pixels with opacity up to 0.998
    white = np.all(rgb == 1.0, axis=2)
    assert white[:20].mean() > 0.95 and (opacity[:20][white[:20]] < 1e-3).all()
    print(f"white pixels {white.mean():.3f}, of them opacity < 1e-3: {(opacity[white] < 1e-3).mean():.3f}; "
          f"opacity max {opacity.max():.8f}, depth max {depth.max():.4f}")
    g = golden(FIX)
    for name in ("centre", "silhouette"):           # a window's maps are the same pixels of the whole frame
        x0, y0, w, h = (int(v) for v in g[f"{name}_crop"])
        _, d, o = _aux(native, renderer, cam800, seed=0, crop=(x0, y0, w, h))
        assert np.array_equal(d, depth[y0:y0 + h, x0:x0 + w]) and np.array_equal(o, opacity[y0:y0 + h, x0:x0 + w])
    plain = native.render_image(renderer.coarse, renderer.fine, cam800, 128, seed=0)
    assert np.array_equal(plain, rgb)


# ---- 7. SSAA and the CLI ---------------------------------------------------------------------------------------------------------
def test_ssaa_maps_are_box_means_of_sub_rays(native, renderer, samples, cam800):
    cam400 = native.camera_from_samples(samples, 400, 400, 64)
    x0, y0, w, h = 192, 184, 16, 16
    got = _aux(native, renderer, cam400, seed=0, crop=(x0, y0, w, h), ssaa=2)
    sub = _aux(native, renderer, cam800, seed=0, crop=(2 * x0, 2 * y0, 2 * w, 2 * h))
    for a, s in zip(got, sub):                       # sum over the 2 x 2 sub-rays, row-major, then * 1/4 (k_box_downsample)
        m = ((s[0::2, 0::2] + s[0::2, 1::2]) + s[1::2, 0::2]) + s[1::2, 1::2]
        assert np.array_equal(a, m * np.float32(0.25))
    _gate(got[0], golden("crop_ssaa2_400.npz")["image"])


def _read_pfm(path):
    raw = open(path, "rb").read()
    head, dims, scale, data = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert head == b"Pf" and float(scale) < 0
    return np.frombuffer(data, "<f4").reshape(h, w)[::-1]


def test_cli_writes_the_library_maps(native, renderer, samples, tmp_path):
    exe = os.path.join(ROOT, "nerf-rs_amd", "nerf_cli")
    cam = native.camera_from_samples(samples, 256, 256, 64)
    rgb, depth, opacity = _aux(native, renderer, cam, seed=0)
    plain = subprocess.run([exe, "--scene", SCENE, "--out", str(tmp_path / "a.ppm")], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    for extra in ([], ["--devices", "0,0", "--gather", "rccl"]):
        d, o = tmp_path / f"d{len(extra)}.pfm", tmp_path / f"o{len(extra)}.pfm"
        res = subprocess.run([exe, "--scene", SCENE, "--out", str(tmp_path / "b.ppm"), "--depth", str(d), "--opacity", str(o)] + extra,
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert np.array_equal(_read_pfm(d), depth) and np.array_equal(_read_pfm(o), opacity)
        assert (tmp_path / "b.ppm").read_bytes() == (tmp_path / "a.ppm").read_bytes()
    strip = lambda s: [l for l in s.splitlines() if "seconds" not in l and "rays/s" not in l]  # noqa: E731 (timings differ run to run)
    assert strip(res.stdout)[:3] == strip(plain.stdout)[:3]
