"""Certified ray batches (nerf_render_rays_certified, nerf_render_rays_clipped_certified, their _device forms; -m gpu): zero certification
inside every pass of a batch.  "Identical" is np.array_equal on the uint32 views of rgb, depth and opacity against the UNCERTIFIED call
on the same context and arguments.

  1. a 40 x 40 lego camera's rays from the shared origin: three arithmetics x four sample plans; with rng_index = row * nx + col also
     render_image(aux=True, certify_zero=True); the lists, and with them n_exec_* and the audit, are those of the certified image;
  2. per-ray origins and bounds (a displaced batch): identical, the audit has nothing to say (a pre-filter that ignored ray_origins would
     certify the wrong samples); one origin repeated == n_origins = 1, bits and lists;
  3. 1, 63, 65, 130 rays at 3 + 5 and 20 + 50 samples; passes of 13 and 50 rays that end inside the batch; a permuted batch;
  4. the retry loop: margins that widen (dense7 x 40) and the bf16 pre-filter (a network beyond the f16 range), on displaced rays;
  5. nerf_stage_prefilter_rays: row r == nerf_stage_prefilter on ray r alone from origins[r], bit patterns, f16 and bf16;
  6. clipped + certified == clipped, bounds / hit flags / scatter / n_hit included, and the empty grid;
  7. the device entry points on torch tensors (a child process); 8. nerf_cli --rays --certify-zero; 9. image renders do not notice."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import certify_batch_cases as CB  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W = 40
DTYPES = ["f32", "f16x2", "bf16x3"]
PLANS = [(64, 128, False), (20, 50, False), (3, 5, False), (64, 0, True)]
PLAN_IDS = ["64+128", "20+50", "3+5", "coarse-only 64"]
FLOORS_F16 = (0.25, 0.5)   # nerf_internal.h kCertMargin*F16: lego fits the f16 range, the pre-filter runs in f16
FLOORS_BF16 = (1.0, 3.0)
SEED = 7
KEYS = ("rgb", "depth", "opacity")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _diff(got, want, what=""):
    out = []
    for k, g, w in zip(KEYS, got, want):
        g, w = np.asarray(g), np.asarray(w).reshape(np.shape(g))
        bad = _bits(g) != _bits(w)
        if bad.any():
            out.append(f"{what} {k}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}")
    return "\n".join(out)


def _pair(native, r, origins, dirs, near, far, nf, **kw):
    """(uncertified (rgb, depth, opacity), certified triple, certified stats) of one batch on one context."""
    plain = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, normalize=False, **kw)
    *cert, st = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, normalize=False, certify_zero=True, return_stats=True, **kw)
    return plain, cert, st


@pytest.fixture(scope="module")
def cam_rays(native, renderer, samples):
    cam = native.camera_from_samples(samples, W, W, 64)
    origin, dirs, near, far, pix = CB.camera_batch(renderer, cam, W)
    for a in (origin, dirs, pix):
        a.setflags(write=False)
    return dict(origin=origin, dirs=dirs, near=near, far=far, pix=pix)


@pytest.fixture(scope="module")
def displaced(cam_rays):
    origins, bounds = CB.displace(cam_rays["origin"], cam_rays["dirs"], cam_rays["near"], cam_rays["far"])
    origins.setflags(write=False); bounds.setflags(write=False)
    return dict(origins=origins, dirs=cam_rays["dirs"], bounds=bounds)


# ---- 1. a camera's rays, shared origin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc,nf,coarse_only", PLANS, ids=PLAN_IDS)
def test_camera_batch_shared_origin(native, renderer, samples, cam_rays, nc, nf, coarse_only, dtype):
    c = cam_rays
    kw = dict(n_coarse=nc, rng_index=c["pix"], seed=SEED, coarse_only=coarse_only, dtype=dtype)
    plain, cert, st = _pair(native, renderer, c["origin"], c["dirs"], c["near"], c["far"], nf, **kw)
    assert not (plain[0] == 1.0).all() and (plain[0] == 1.0).all(axis=1).any()          # rays through the model and empty rays, both
    assert not _diff(cert, plain, "certified vs plain")
    cam = native.camera_from_samples(samples, W, W, nc)
    *img, ist = native.render_image(renderer.coarse, renderer.fine, cam, nf, seed=SEED, coarse_only=coarse_only, dtype=dtype, aux=True,
                                    certify_zero=True, return_stats=True)
    assert not _diff(cert, [img[0].reshape(-1, 3), img[1].reshape(-1), img[2].reshape(-1)], "certified batch vs certified image")
    assert st.n_rays == W * W and st.n_passes == ist.n_passes == 1
    assert st.n_certify_violations == 0 and st.n_certify_retries == 0 and st.certify_margin == FLOORS_F16
    # one pass, the same seed, the same pre-filter and plan: the lists are the image's, entry for entry
    assert (st.n_exec_coarse_trunk, st.n_exec_fine_trunk, st.n_certify_audited) == (ist.n_exec_coarse_trunk, ist.n_exec_fine_trunk, ist.n_certify_audited)
    if dtype == "f32" and (nc, nf) == (64, 128):
        print(f"\ncertified 40 x 40 batch: coarse {st.n_exec_coarse_trunk} of {st.n_coarse_points}, fine {st.n_exec_fine_trunk} of {st.n_fine_points}, "
              f"audited {st.n_certify_audited}, headroom {st.certify_headroom}")
        assert st.n_exec_fine_trunk < st.n_fine_points and st.n_exec_coarse_trunk < st.n_coarse_points


# ---- 2. per-ray origins and bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_per_ray_origins_and_bounds(native, renderer, displaced, dtype):
    d = displaced
    plain, cert, st = _pair(native, renderer, d["origins"], d["dirs"], 0.0, 0.0, 128, bounds=d["bounds"], seed=SEED, dtype=dtype)
    assert not (plain[0] == 1.0).all() and (plain[0] == 1.0).all(axis=1).any()
    assert not _diff(cert, plain, "displaced batch")
    # the audit evaluates certified samples exactly: certificates made for the wrong points would show here
    assert st.n_certify_audited > 0 and st.n_certify_retries == 0 and st.n_certify_violations == 0 and st.certify_margin == FLOORS_F16
    assert all(h >= 0.5 * m for h, m in zip(st.certify_headroom, st.certify_margin))
    assert st.n_exec_fine_trunk < 0.5 * st.n_fine_points and st.n_exec_coarse_trunk < 0.6 * st.n_coarse_points


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_origin_is_the_shared_origin(native, renderer, cam_rays, dtype):
    c = cam_rays
    kw = dict(n_coarse=20, rng_index=c["pix"], seed=SEED, dtype=dtype, aux=True, normalize=False, certify_zero=True, return_stats=True)
    *shared, s0 = native.render_rays(renderer.coarse, renderer.fine, c["origin"], c["dirs"], c["near"], c["far"], 50, **kw)
    *per_ray, s1 = native.render_rays(renderer.coarse, renderer.fine, np.tile(c["origin"], (len(c["dirs"]), 1)), c["dirs"], c["near"], c["far"], 50, **kw)
    assert not _diff(per_ray, shared, "repeated origin")
    assert (s1.n_exec_coarse_trunk, s1.n_exec_fine_trunk, s1.n_exec_colour, s1.n_certify_audited) == \
           (s0.n_exec_coarse_trunk, s0.n_exec_fine_trunk, s0.n_exec_colour, s0.n_certify_audited)
    assert 0 < s0.n_exec_fine_trunk < s0.n_fine_points


# ---- 3. shapes that align with nothing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,nf", [(3, 5), (20, 50)])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_odd_ray_counts(native, renderer, displaced, n, nc, nf):
    d = displaced
    pick = np.arange(n) * 11 + 60                                                        # across the frame, model and background
    for dtype in DTYPES:
        plain, cert, st = _pair(native, renderer, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, nf, n_coarse=nc, bounds=d["bounds"][pick],
                                rng_index=pick, seed=SEED, dtype=dtype)
        assert not _diff(cert, plain, f"{n} rays {nc}+{nf} {dtype}")
        assert st.n_rays == n and st.n_certify_violations == 0


@pytest.mark.parametrize("per_pass", [13, 50])
def test_passes_end_inside_the_batch(native, displaced, monkeypatch, per_pass):
    """NERF_MAX_RAYS_PER_PASS is read when a context is created: the list, its counters and the audit salt are per pass."""
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(per_pass))
    d = displaced
    pick = np.arange(130) * 11 + 100
    with native.Renderer(0) as r:
        r.load_scene(SCENE)
        for dtype in ("f32", "f16x2"):
            plain, cert, st = _pair(native, r, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, 50, n_coarse=20, bounds=d["bounds"][pick], seed=SEED, dtype=dtype)
            assert not _diff(cert, plain, f"passes of {per_pass} {dtype}")
            assert st.n_passes == -(-130 // per_pass) and st.n_certify_violations == 0 and st.n_certify_retries == 0
            assert 0 < st.n_exec_fine_trunk < st.n_fine_points


def test_fused_prefilter_setting(native, cam_rays, displaced, monkeypatch):
    """NERF_CERTIFY_SEQ_PREFILTER=0 (read when a context is created): the fused 16-bit pre-filter serves a shared origin; it knows one
    origin only, so a pass with per-ray origins takes the ray-sequential pre-filter all the same -- identical either way."""
    monkeypatch.setenv("NERF_CERTIFY_SEQ_PREFILTER", "0")
    c, d = cam_rays, displaced
    pick = np.arange(130) * 11 + 100
    with native.Renderer(0) as r:
        r.load_scene(SCENE)
        plain, cert, st = _pair(native, r, c["origin"], c["dirs"][pick], c["near"], c["far"], 50, n_coarse=20, rng_index=pick, seed=SEED)
        assert not _diff(cert, plain, "fused pre-filter, shared origin") and st.n_certify_violations == 0 and st.n_certify_retries == 0
        plain, cert, st = _pair(native, r, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, 50, n_coarse=20, bounds=d["bounds"][pick], seed=SEED)
        assert not _diff(cert, plain, "per-ray origins under the fused setting") and st.n_certify_violations == 0 and st.n_certify_retries == 0
        assert 0 < st.n_exec_fine_trunk < st.n_fine_points


def test_a_permuted_batch_permutes_the_outputs(native, renderer, displaced):
    d = displaced
    n = len(d["dirs"])
    perm = np.random.default_rng(3).permutation(n)
    kw = dict(n_coarse=20, seed=SEED, aux=True, normalize=False, certify_zero=True)
    base = native.render_rays(renderer.coarse, renderer.fine, d["origins"], d["dirs"], 0.0, 0.0, 50, bounds=d["bounds"], rng_index=np.arange(n), **kw)
    mixed = native.render_rays(renderer.coarse, renderer.fine, d["origins"][perm], d["dirs"][perm], 0.0, 0.0, 50, bounds=d["bounds"][perm], rng_index=perm, **kw)
    assert not _diff(mixed, [a[perm] for a in base], "permuted")


# ---- 4. the retry loop -----------------------------------------------------------------------------------------------------------------------
def _load(native, r, root):
    r.coarse = native.load_network_from_dir(r, 0, os.path.join(root, "coarse"))
    r.fine = native.load_network_from_dir(r, 1, os.path.join(root, "fine"))


def test_margins_widen_on_a_batch(native, displaced, tmp_path):
    d = displaced
    pick = np.arange(600) * 2 + 200
    with native.Renderer(0) as r:
        _load(native, r, CB.scaled_lego(SCENE, str(tmp_path / "hot"), 40.0))
        plain, cert, st = _pair(native, r, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, 128, bounds=d["bounds"][pick], seed=3)
        print(f"\nhot network, batch: {st.n_certify_retries} retries, {st.n_certify_violations} violations seen, margins {st.certify_margin}")
        assert not _diff(cert, plain, "hot network")
        assert st.n_certify_retries > 0 or any(m > f for m, f in zip(st.certify_margin, FLOORS_F16))
        plain2, cert2, st2 = _pair(native, r, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, 128, bounds=d["bounds"][pick], seed=4)
        assert not _diff(cert2, plain2, "hot network, next batch")
        assert all(b >= a for a, b in zip(st.certify_margin, st2.certify_margin))       # margins never come back within a context


def test_beyond_the_f16_range_uses_the_bf16_prefilter(native, displaced, tmp_path):
    """The f16 pre-filter leaves its range, the batch is rendered again behind nerf_trunk_seq_kernel_bf16 with ray_origins."""
    d = displaced
    pick = np.arange(600) * 2 + 200
    with native.Renderer(0) as r:
        _load(native, r, CB.beyond_f16_lego(SCENE, str(tmp_path / "big")))
        plain, cert, st = _pair(native, r, d["origins"][pick], d["dirs"][pick], 0.0, 0.0, 128, bounds=d["bounds"][pick], seed=3)
        print(f"\nbeyond the f16 range, batch: {st.n_certify_retries} retries, margins {st.certify_margin}")
        assert not _diff(cert, plain, "beyond f16")
        assert st.n_certify_retries >= 1 and all(m >= f for m, f in zip(st.certify_margin, FLOORS_BF16))


# ---- 5. the pre-filter's origin routing, stage level -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spr", [40, 192])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_stage_prefilter_rays_routes_each_origin_to_its_ray(native, renderer, displaced, kind, spr):
    d = displaced
    pick = np.arange(8) * 190 + 60
    o, dirs, b = d["origins"][pick], d["dirs"][pick], d["bounds"][pick]
    assert len({tuple(x) for x in o}) == 8
    u = (np.arange(spr, dtype=F) + F(0.5)) / F(spr)
    t = (b[:, :1] + (b[:, 1:] - b[:, :1]) * u[None, :]).astype(F)
    for which in (0, 1):
        for cut_T in (0.0, 0.01):
            rows, bad = renderer.stage_prefilter(which, None, dirs, t, 6.0, f16=kind == "f16", cut_T=cut_T, origins=o)
            assert bad == 0
            for k in range(8):
                one, _ = renderer.stage_prefilter(which, o[k], dirs[k:k + 1], t[k:k + 1], 6.0, f16=kind == "f16", cut_T=cut_T)
                assert np.array_equal(_bits(rows[k]), _bits(one[0])), (which, cut_T, k)     # NaN "not evaluated" entries included
            other, _ = renderer.stage_prefilter(which, o[0], dirs, t, 6.0, f16=kind == "f16", cut_T=cut_T)
            assert np.array_equal(_bits(other[0]), _bits(rows[0])) and not np.array_equal(_bits(other[1:]), _bits(rows[1:]))


# ---- 6. clipped + certified ------------------------------------------------------------------------------------------------------------------
LEGO_LO, LEGO_DIMS = (-1.3, -1.3, -0.8), (32, 32, 32)
LEGO_STEP = (2.6 / 32, 2.6 / 32, 2.2 / 32)


def test_clipped_and_certified(native, renderer, samples):
    _, bits, count, _ = renderer.fine.density_grid(LEGO_LO, LEGO_STEP, LEGO_DIMS, threshold=1.0, want_sigma=False)
    grown = native.dilate_occupancy(renderer, bits, LEGO_DIMS, 1)
    cam = native.camera_from_samples(samples, 24, 24, 16)
    dirs = renderer.stage_ray_dirs(cam, 0, 0, 24, 24, normalize=True).reshape(-1, 3)
    n = len(dirs)
    origin = np.asarray(cam.pos, F)
    origins, bounds = CB.displace(origin, dirs, cam.near, cam.far, seed=5)
    grid = (LEGO_LO, LEGO_STEP, LEGO_DIMS)
    cases = [("shared origin", grown, origin, dict()), ("per-ray origins, own bounds", grown, origins, dict(bounds=bounds)),
             ("another background", grown, origins, dict(bounds=bounds, background=(0.25, 0.5, 0.75), rng_index=np.arange(n)[::-1].copy())),
             ("f16x2", grown, origins, dict(bounds=bounds, dtype="f16x2")), ("empty grid", np.zeros_like(grown), origin, dict())]
    for what, g, o, kw in cases:
        kw = dict(n_coarse=16, seed=SEED, aux=True, normalize=False, return_hit=True, **kw)
        plain = native.render_rays_clipped(renderer.coarse, renderer.fine, g, *grid, o, dirs, cam.near, cam.far, 32, **kw)
        *cert, st = native.render_rays_clipped(renderer.coarse, renderer.fine, g, *grid, o, dirs, cam.near, cam.far, 32, certify_zero=True, return_stats=True, **kw)
        assert not _diff(cert[:3], plain[:3], what)
        assert np.array_equal(cert[3], plain[3]) and cert[4] == plain[4] == int(plain[3].sum()), what
        if what == "empty grid":
            assert cert[4] == 0 and st.n_rays == 0
        else:
            assert 40 < cert[4] < n and st.n_rays == cert[4] and st.n_certify_violations == 0 and st.n_certify_retries == 0
            assert 0 < st.n_exec_fine_trunk < st.n_fine_points


# ---- 7. the device entry points on torch tensors ---------------------------------------------------------------------------------------------
def test_device_entry_points_on_torch_tensors():
    """tests/helpers/ray_batch_certify_torch_child.py: a process of its own, because it must load torch's HIP runtime before the library's."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ray_batch_certify_torch_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok 14", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


# ---- 8. the command-line tool ----------------------------------------------------------------------------------------------------------------
def test_cli_certified_rays_write_the_same_bytes(native, tmp_path):
    rng = np.random.default_rng(5)
    n = 117
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(F)
    d = (rng.uniform(-0.8, 0.8, (n, 3)).astype(F) - o).astype(F)
    np.hstack([o, d]).astype("<f4").tofile(tmp_path / "rays.f32")
    cli = [os.path.join(os.path.dirname(native.lib_path()), "nerf_cli"), "--scene", SCENE, "--rays", str(tmp_path / "rays.f32"), "--coarse", "20", "--fine", "50",
           "--seed", "9"]
    p = subprocess.run(cli + ["--rays-out", str(tmp_path / "plain.f32")], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0 and "certify_zero audit" not in p.stdout, (p.stdout, p.stderr)
    p = subprocess.run(cli + ["--rays-out", str(tmp_path / "cert.f32"), "--certify-zero"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0 and "117 rays (20 coarse + 50 fine samples)" in p.stdout and "certify_zero audit:" in p.stdout and ", 0 violations," in p.stdout, (p.stdout, p.stderr)
    plain, cert = (tmp_path / "plain.f32").read_bytes(), (tmp_path / "cert.f32").read_bytes()
    assert len(plain) == 12 * n and cert == plain
    rgb = np.frombuffer(plain, "<f4").reshape(n, 3)
    assert (rgb == 1.0).all(axis=1).any() and not (rgb == 1.0).all()


# ---- 9. image renders do not notice -----------------------------------------------------------------------------------------------------------
def test_image_renders_do_not_notice_a_certified_batch(native, renderer, samples, displaced):
    cam = native.camera_from_samples(samples, 800, 800, 64)
    crop = (311, 287, 13, 9)
    d = displaced
    renderer.kernel_time_query(reset=True)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    _, _, launches = renderer.kernel_time_query(reset=False)
    for dtype in ("f32", "bf16x3"):
        native.render_rays(renderer.coarse, renderer.fine, d["origins"], d["dirs"], 0.0, 0.0, 128, bounds=d["bounds"], seed=SEED, dtype=dtype, certify_zero=True)
    ms, points, after_batch = renderer.kernel_time_query(reset=False)
    assert after_batch == launches == 1 and points == 13 * 9 * 192
    after = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    assert not _diff([a.reshape(-1) for a in after], [b.reshape(-1) for b in before], "crop render")
    assert renderer.kernel_time_query(reset=True)[2] == 2
