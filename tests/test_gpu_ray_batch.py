"""render_rays -- the caller's rays instead of a camera's (nerf_render_rays, nerf_render_rays_device; -m gpu).  Equalities are bit for bit.

  1. a batch made of a camera's rays IS render_image(aux=True) of that window: colour, depth, opacity; unit directions with normalize=0
     and raw directions with normalize=1; three lego windows x eight sample shapes x four arithmetics;
  2. per-ray origins (k_batch_points + points-mode launches) with one origin repeated == the shared-origin path (ray-mode launches);
  3. permuting a batch, rng_index along with it, permutes its outputs; rng_index=None is arange;
  4. a batch no camera can make -- displaced origins, three (near, far) pairs -- == tests/helpers/ray_batch_restatement.restate_rays
     on the product's own stage calls (checked against the oracle on the CPU: tests/test_ray_batch_restatement_cpu.py);
  5. that batch and the probe batch against the ORACLE's networks and integrate_ray at the restatement's own sample positions, at the
     project's unrelaxed Gate 1 (max <= 5e-4, mean <= 1e-5, PSNR >= 90 dB);
  6. the mutant restatement of the probe batch (sample 0 of every ray given the previous ray's direction) fails both;
  7. 1, 63, 65, 117 and 130 rays at 3 + 5 and 20 + 50 samples (rays x samples and the 3-float stores aligned with nothing), and passes
     of 13 and 50 rays that end inside the batch;
  8. another background; the device entry point on torch tensors; image renders and their kernel-time bookkeeping untouched by a batch;
     nerf_cli --rays."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import SCENE, psnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402
from test_gpu_render_restatement import DTYPES, LEGO_SEED, LEGO_WINDOWS, SHAPES  # noqa: E402  (the shapes and windows, not its tests)

pytestmark = pytest.mark.gpu

KEYS = ("rgb", "depth", "opacity")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _diff(got, want, what=""):
    """'' if the (rgb, depth, opacity) triple `got` carries the bits of `want` (a triple, or a restatement dict), else what differs."""
    want = [want[k] for k in KEYS] if isinstance(want, dict) else list(want)
    out = []
    for k, g, w in zip(KEYS, got, want):
        g, w = np.asarray(g), np.asarray(w).reshape(np.shape(g))
        bad = _bits(g) != _bits(w)
        if bad.any():
            out.append(f"{what} {k}: {int(bad.sum())} of {bad.size} values differ, max {np.abs(g.astype(np.float64) - w).max():.3e}, first at {tuple(np.argwhere(bad)[0])}")
    return "\n".join(out)


def _gate1(img, ref):
    d = np.abs(img - ref)
    return d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(img, ref) >= 90.0


def _rays(native, r, origins, dirs, near, far, nf, **kw):
    return native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, **kw)


# ---- 1. a camera's rays -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc,nf,coarse_only", SHAPES, ids=[f"{a}+{b}" if not c else f"coarse-only {a}" for a, b, c in SHAPES])
def test_camera_batch_is_the_image_render(native, renderer, samples, nc, nf, coarse_only, dtype):
    be = RR.GpuBackend(native, renderer)
    failures, white = [], []
    for W, crop in LEGO_WINDOWS:
        cam = native.camera_from_samples(samples, W, W, nc)
        want = native.render_image(renderer.coarse, renderer.fine, cam, nf, seed=LEGO_SEED, crop=crop, coarse_only=coarse_only, dtype=dtype, aux=True)
        origin, unit, near, far, pix = RB.camera_batch(be, cam, crop)
        raw = renderer.stage_ray_dirs(cam, *crop, normalize=False).reshape(-1, 3)
        assert not np.array_equal(_bits(raw), _bits(unit))
        kw = dict(n_coarse=nc, rng_index=pix, seed=LEGO_SEED, coarse_only=coarse_only, dtype=dtype)
        failures.append(_diff(_rays(native, renderer, origin, unit, near, far, nf, normalize=False, **kw), want, f"{W}^2 {crop} unit dirs"))
        failures.append(_diff(_rays(native, renderer, origin, raw, near, far, nf, normalize=True, **kw), want, f"{W}^2 {crop} raw dirs"))
        white.append((want[0] == 1.0).all(axis=2).reshape(-1))
    white = np.concatenate(white)
    assert white.any() and not white.all()          # empty rays and rays through the model, both
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


# ---- 2. the two paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_origin_is_the_shared_origin_path(native, renderer, samples, dtype):
    be = RR.GpuBackend(native, renderer)
    W, crop = LEGO_WINDOWS[0]
    failures = []
    for nc, nf, coarse_only in SHAPES:
        cam = native.camera_from_samples(samples, W, W, nc)
        origin, unit, near, far, pix = RB.camera_batch(be, cam, crop)
        kw = dict(n_coarse=nc, rng_index=pix, seed=LEGO_SEED, coarse_only=coarse_only, dtype=dtype, normalize=False)
        shared = _rays(native, renderer, origin, unit, near, far, nf, **kw)
        per_ray = _rays(native, renderer, np.tile(origin, (len(unit), 1)), unit, near, far, nf, **kw)
        assert not (shared[0] == 1.0).all()
        failures.append(_diff(per_ray, shared, f"{nc}+{nf} coarse_only={coarse_only}"))
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


# ---- the probe and the displaced batch ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(native, oracle, samples, tmp_path_factory):
    P = RR.PROBE
    root = RR.probe_scene(tmp_path_factory.mktemp("probe") / "scene")
    r = native.Renderer(0)
    r.load_scene(str(root))
    n = P["size"]
    be = RR.GpuBackend(native, r)
    cam = native.camera_from_samples(samples, n, n, P["nc"])
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, (0, 0, n, n))
    p = types.SimpleNamespace(r=r, be=be, origin=origin, dirs=dirs, near=near, far=far, pix=pix, nc=P["nc"], nf=P["nf"], seed=P["seed"],
                              onets=(oracle.Net(str(root / "coarse")), oracle.Net(str(root / "fine"))), cache={})

    def restated(dtype, mutant=False):
        key = (dtype, mutant)
        if key not in p.cache:
            rs = RB.restate_rays(be, origin, dirs, near, far, None, pix, p.nc, p.nf, p.seed, False, dtype,
                                 fine_dirs=RR.roll_first_sample if mutant else None)
            for a in rs.values():
                a.setflags(write=False)
            p.cache[key] = rs
        return p.cache[key]

    p.restated = restated
    p.render = lambda dtype, **kw: _rays(native, r, origin, dirs, near, far, p.nf, n_coarse=p.nc, rng_index=pix, seed=p.seed, dtype=dtype,
                                         normalize=False, **kw)
    yield p
    r.close()


@pytest.fixture(scope="module")
def displaced(native, renderer, samples):
    D = RB.DISPLACED
    be = RR.GpuBackend(native, renderer)
    cam = native.camera_from_samples(samples, D["W"], D["W"], D["nc"])
    origins, dirs, bounds = RB.displaced_batch(be, cam, D["crop"])
    d = types.SimpleNamespace(be=be, origins=origins, dirs=dirs, bounds=bounds, nc=D["nc"], nf=D["nf"], seed=D["seed"], cache={})

    def restated(dtype, background=None):
        key = (dtype, None if background is None else tuple(background))
        if key not in d.cache:
            rs = RB.restate_rays(be, origins, dirs, 0.0, 0.0, bounds, None, d.nc, d.nf, d.seed, False, dtype, background=background)
            for a in rs.values():
                a.setflags(write=False)
            d.cache[key] = rs
        return d.cache[key]

    d.restated = restated
    # near_ / far_ are not read when bounds are given: NaN would show if they were
    d.render = lambda r, dtype, **kw: _rays(native, r, origins, dirs, float("nan"), float("nan"), d.nf, n_coarse=d.nc, bounds=bounds, seed=d.seed,
                                            dtype=dtype, normalize=False, **kw)
    return d


# ---- 3. permutation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_permuting_a_batch_permutes_its_outputs(native, renderer, probe, displaced, dtype):
    perm = np.random.default_rng(20240607).permutation(144)
    assert (perm != np.arange(144)).mean() > 0.9
    base = probe.render(dtype)
    got = _rays(native, probe.r, probe.origin, probe.dirs[perm], probe.near, probe.far, probe.nf, n_coarse=probe.nc, rng_index=probe.pix[perm],
                seed=probe.seed, dtype=dtype, normalize=False)
    assert not _diff(got, [a[perm] for a in base], "probe")
    assert len({tuple(v) for v in _bits(base[0]).tolist()}) > 100           # the rays differ: a permutation that was ignored would show
    # the 117-ray lego batch with per-ray origins and bounds: everything of a ray travels with it
    d = displaced
    perm = np.random.default_rng(7).permutation(len(d.dirs))
    idx = np.arange(len(d.dirs), dtype=np.uint32)
    base = d.render(renderer, dtype)
    got = _rays(native, renderer, d.origins[perm], d.dirs[perm], 0.0, 0.0, d.nf, n_coarse=d.nc, bounds=d.bounds[perm], rng_index=idx[perm],
                seed=d.seed, dtype=dtype, normalize=False)
    assert not _diff(got, [a[perm] for a in base], "lego")
    assert not _diff(d.render(renderer, dtype, rng_index=idx), base, "rng_index = arange")      # None: ray r draws from index r


# ---- 4. per-ray origins and bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_displaced_origins_and_bounds_are_their_restatement(renderer, displaced, dtype):
    rs = displaced.restated(dtype)
    white = (rs["rgb"] == 1.0).all(axis=1)
    assert white.any() and not white.all()          # tests/test_ray_batch_restatement_cpu.py holds the same of the oracle
    assert len(RB._groups(rs["far"])) == 3
    got = displaced.render(renderer, dtype)
    assert np.isfinite(got[0]).all()
    assert not _diff(got, rs, dtype)


# ---- 5. the oracle ------------------------------------------------------------------------------------------------------------------------
def _oracle_on_samples(oracle, net, rs):
    """oracle fine network at the restatement's float32 points with each ray's direction, composited by oracle.integrate_ray to the ray's far."""
    R, n = rs["t_fine"].shape
    rgb, sg = net.forward_batch(rs["pts_fine"], np.repeat(rs["dirs"], n, axis=0))
    rgb, sg = rgb.reshape(R, n, 3), sg.reshape(R, n)
    return np.stack([oracle.integrate_ray(rgb[r], sg[r], rs["t_fine"][r], float(rs["far"][r])) for r in range(R)])


@pytest.fixture(scope="module")
def oracle_refs(oracle, oracle_nets, probe, displaced):
    """{batch: {dtype: reference}}: computed once per restatement (bf16x3 and f16x2 share f32's sample positions but are asked separately)."""
    return dict(cache={}, nets=dict(probe=probe.onets[1], lego=oracle_nets[1]))


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("which", ["lego", "probe"])
def test_batches_against_the_oracle_on_their_own_samples(native, oracle, renderer, probe, displaced, oracle_refs, which, dtype):
    """Measured on an MI355X: see the figures printed below (recorded in DESIGN 4.13)."""
    rs = displaced.restated(dtype) if which == "lego" else probe.restated(dtype)
    key = (which, _bits(rs["pts_fine"]).tobytes())
    if key not in oracle_refs["cache"]:
        oracle_refs["cache"][key] = _oracle_on_samples(oracle, oracle_refs["nets"][which], rs)
    ref = oracle_refs["cache"][key]
    img = (displaced.render(renderer, dtype) if which == "lego" else probe.render(dtype))[0]
    d = np.abs(img - ref)
    print(f"\n{which} batch {dtype} vs the oracle on the batch's samples: max {d.max():.3e} mean {d.mean():.3e} psnr {psnr(img, ref):.1f} dB")
    assert _gate1(img, ref), (which, dtype, d.max(), d.mean(), psnr(img, ref))


# ---- 6. the mutant ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16x2"])
def test_probe_batch_is_its_restatement_and_not_the_mutant(oracle, probe, oracle_refs, dtype):
    rs, mutant = probe.restated(dtype), probe.restated(dtype, mutant=True)
    for k in ("t_coarse", "sigma_coarse", "t_fine", "sigma_fine", "w_fine", "depth", "opacity"):      # the mutant differs in colours alone
        assert np.array_equal(_bits(rs[k]), _bits(mutant[k])), k
    got = probe.render(dtype)
    assert not _diff(got, rs, "probe")
    assert (_bits(got[0]) != _bits(mutant["rgb"])).any(axis=1).mean() > 0.5             # ONE wrong direction per ray: the equality fails
    ref = _oracle_on_samples(oracle, probe.onets[1], rs)
    d = np.abs(mutant["rgb"] - ref)
    print(f"\nmutant restatement {dtype} vs the oracle: max {d.max():.3e} mean {d.mean():.3e}, {(d.max(axis=1) > 5e-4).mean():.2f} of the rays above 5e-4")
    assert _gate1(got[0], ref) and not _gate1(mutant["rgb"], ref)                      # ... and so does Gate 1


def test_probe_bf16_batch_is_its_restatement(probe):
    assert not _diff(probe.render("bf16"), probe.restated("bf16"), "probe bf16")


# ---- 7. shapes and passes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(native, renderer, samples):
    """130 rays (a 13 x 10 window) with displaced origins and cycling bounds, restated once per sample shape."""
    be = RR.GpuBackend(native, renderer)
    cam = native.camera_from_samples(samples, 800, 800, 20)
    origins, dirs, bounds = RB.displaced_batch(be, cam, (311, 286, 13, 10))
    rs = {(nc, nf): RB.restate_rays(be, origins, dirs, 0.0, 0.0, bounds, None, nc, nf, 11, False, "f32") for nc, nf in ((3, 5), (20, 50))}
    return origins, dirs, bounds, rs


@pytest.mark.parametrize("n", [1, 63, 65, 117, 130])
@pytest.mark.parametrize("nc,nf", [(3, 5), (20, 50)])
def test_ray_counts_that_align_with_nothing(native, renderer, ragged, nc, nf, n):
    origins, dirs, bounds, rs = ragged
    want = [rs[(nc, nf)][k][:n] for k in KEYS]
    kw = dict(n_coarse=nc, bounds=bounds[:n], seed=11, normalize=False)
    assert not _diff(_rays(native, renderer, origins[:n], dirs[:n], 0.0, 0.0, nf, **kw), want, "per-ray origins")
    for dtype in DTYPES:        # one origin for every ray: ray-mode launches == points-mode launches over the expanded samples
        shared = _rays(native, renderer, origins[0], dirs[:n], 0.0, 0.0, nf, dtype=dtype, **kw)
        per_ray = _rays(native, renderer, np.tile(origins[0], (n, 1)), dirs[:n], 0.0, 0.0, nf, dtype=dtype, **kw)
        assert not _diff(per_ray, shared, f"{dtype} repeated origin")


@pytest.mark.parametrize("cap", [13, 50])
def test_passes_that_end_inside_the_batch(native, renderer, displaced, monkeypatch, cap):
    """NERF_MAX_RAYS_PER_PASS (read when a context is created): 117 rays in 9 passes of 13 and in 3 passes of 50, 50 and 17 -- a pass re-bases
    rays, outputs, bounds and the default RNG index; the one-pass render and the restatement know nothing of passes."""
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(cap))
    n = len(displaced.dirs)
    with native.Renderer(0) as r2:
        r2.load_scene(SCENE)
        for dtype in DTYPES:
            got = displaced.render(r2, dtype, return_stats=True)
            assert got[3].n_passes == -(-n // cap) and got[3].n_rays == n
            assert not _diff(got[:3], displaced.render(renderer, dtype), f"cap {cap} {dtype}")
        assert not _diff(displaced.render(r2, "f32"), displaced.restated("f32"), f"cap {cap} restatement")
        shared = _rays(native, r2, displaced.origins[0], displaced.dirs, 2.0, 6.0, displaced.nf, n_coarse=displaced.nc, seed=displaced.seed)
        assert not _diff(shared, _rays(native, renderer, displaced.origins[0], displaced.dirs, 2.0, 6.0, displaced.nf, n_coarse=displaced.nc,
                                       seed=displaced.seed), f"cap {cap} shared origin")


# ---- 8. the rest ------------------------------------------------------------------------------------------------------------------------
def test_another_background_is_the_restatement_with_it(renderer, displaced):
    bg = (0.25, 0.5, 0.75)
    for dtype in ("f32", "f16x2"):
        rs = displaced.restated(dtype, background=bg)
        got = displaced.render(renderer, dtype, background=bg)
        assert not _diff(got, rs, f"background {dtype}")
        white = displaced.render(renderer, dtype)
        empty = white[2] == 0.0
        assert empty.any() and np.array_equal(got[0][empty], np.tile(np.float32(bg), (int(empty.sum()), 1)))
        assert np.array_equal(_bits(got[1]), _bits(white[1])) and np.array_equal(_bits(got[2]), _bits(white[2]))


def test_stats_and_outputs_without_maps(native, renderer, displaced):
    d = displaced
    rgb, st = native.render_rays(renderer.coarse, renderer.fine, d.origins, d.dirs, 0.0, 0.0, d.nf, n_coarse=d.nc, bounds=d.bounds, seed=d.seed,
                                 normalize=False, return_stats=True)
    n = len(d.dirs)
    assert np.array_equal(_bits(rgb), _bits(d.render(renderer, "f32")[0]))           # the colour is the same bits without the maps
    assert (st.n_rays, st.n_coarse_points, st.n_fine_points, st.n_passes, st.n_mlp_launches) == (n, n * d.nc, n * (d.nc + d.nf), 1, 2)
    assert st.ms_total > 0 and st.ms_fine_mlp > 0 and st.ms_coarse_mlp > 0 and st.n_nonfinite_points == 0
    assert native.render_rays(renderer.coarse, renderer.fine, d.origins[:0], d.dirs[:0], 2.0, 6.0, d.nf).shape == (0, 3)     # a no-op


def test_device_entry_point_on_torch_tensors():
    """tests/helpers/ray_batch_torch_child.py: torch tensors in, torch tensors out, on a torch stream, per-ray and shared origins, f32 and
    bf16x3 -- the bits of the host entry point.  A process of its own, because it must load torch's HIP runtime before the library's (see
    the helper); the interplay with torch is what this test is about."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ray_batch_torch_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok 16", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def test_image_renders_do_not_notice_a_batch(native, renderer, samples, displaced):
    cam = native.camera_from_samples(samples, 800, 800, 64)
    crop = (311, 287, 13, 9)
    renderer.kernel_time_query(reset=True)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    _, _, launches = renderer.kernel_time_query(reset=False)
    for dtype in ("f32", "bf16x3"):
        displaced.render(renderer, dtype)
    ms, points, after_batch = renderer.kernel_time_query(reset=False)
    assert after_batch == launches == 1 and points == 13 * 9 * 192         # the batch's launches are not the image renders' dominant kernel
    after = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    assert not _diff(after, before, "crop render")
    assert renderer.kernel_time_query(reset=True)[2] == 2


# ---- the command-line tool --------------------------------------------------------------------------------------------------------------
def test_cli_rays_are_render_rays(native, renderer, samples, tmp_path):
    """nerf_cli --rays FILE --rays-out FILE [--rays-bounds FILE]: n x 6 f32 in, n x 3 f32 out, near / far from the scene JSON; no image
    is rendered; an option ray batches refuse is the library's error."""
    rng = np.random.default_rng(5)
    n = 117
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)      # a ring of eyes
    d = (rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32) - o).astype(np.float32)                                  # not unit
    b = np.stack([rng.uniform(2.0, 3.0, n), rng.uniform(5.0, 6.0, n)], axis=1).astype(np.float32)
    np.hstack([o, d]).astype("<f4").tofile(tmp_path / "rays.f32")
    b.astype("<f4").tofile(tmp_path / "bounds.f32")
    cli = [os.path.join(os.path.dirname(native.lib_path()), "nerf_cli"), "--scene", SCENE, "--rays", str(tmp_path / "rays.f32"), "--rays-out", str(tmp_path / "rgb.f32")]
    bg = (0.25, 0.5, 0.75)
    p = subprocess.run(cli + ["--rays-bounds", str(tmp_path / "bounds.f32"), "--background", "0.25,0.5,0.75", "--coarse", "20", "--fine", "50", "--seed", "9",
                              "--dtype", "f16x2"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0 and "117 rays (20 coarse + 50 fine samples)" in p.stdout, (p.stdout, p.stderr)
    assert not (tmp_path / "output.ppm").exists()
    got = np.fromfile(tmp_path / "rgb.f32", "<f4").reshape(n, 3)
    want = native.render_rays(renderer.coarse, renderer.fine, o, d, float(samples["near"]), float(samples["far"]), 50, n_coarse=20, bounds=b, seed=9,
                              dtype="f16x2", background=bg)
    assert np.array_equal(_bits(got), _bits(want))
    empty = (want == np.float32(bg)).all(axis=1)
    assert empty.any() and not empty.all()
    p = subprocess.run(cli + ["--ssaa", "2"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 1 and "ssaa must be 0 or 1" in p.stderr
    p = subprocess.run(cli[:-2], capture_output=True, text=True, timeout=120, cwd=tmp_path)          # --rays without --rays-out: usage
    assert p.returncode == 2
