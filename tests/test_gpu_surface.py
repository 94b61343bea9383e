"""Quantile depths and point clouds on the GPU (nerf_render_rays_quantiles, nerf_render_rays_points and the two stage calls; contract:
include/nerf_mi355x.h, "quantile depth and point clouds"): every output is compared BIT FOR BIT with tests/helpers/surface_restatement.py
run on the positions and weights tests/helpers/ray_batch_restatement.py restates from the stage calls, or on synthetic data.

  1. the stage calls on synthetic data: 1 .. 130 rays (the 64-ray wave), 1 .. 512 samples (the 16-sample staging chunk), 1, 3 and 8
     quantiles with exact ties, q = 1, all-zero rays and NaN weights; the compaction at 1 .. 1000 rays (the 256-ray scan block) with
     every third ray missing, none kept, all kept, a capacity one short, shared and per-ray origins;
  2. render_rays(quantiles=...): 1 .. 130 lego rays at 3 + 5, 7 + 10 and 20 + 50 samples with per-ray origins and bounds, a shared origin,
     coarse_only, n_fine = 0, all four arithmetics, rays aimed away from the model, passes that end inside the batch;
  3. the invariants: colour, depth and opacity keep their bits; depth_q != 0 implies opacity >= q; depth_q is monotone in q; a
     permutation permutes; host and device forms agree, on raw device pointers and on torch tensors on a torch stream; image renders do
     not notice;
  4. point_cloud against the helper fed with render_rays over black and render_rays(normals_h=h): count, order, every array; several
     passes (the running offset); n_rays = 0; scaled directions with normalize=True; render_image_points; the command-line tool;
  5. the GPU's quantile depths against the oracle's weights, on the rays the recorded difference of the partial sums decides."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402
import surface_restatement as SR  # noqa: E402
from test_gpu_density import DeviceBuffers  # noqa: E402  (the helper, not its tests)
from test_normal_restatement_cpu import LEGO_NORMALS  # noqa: E402  (the window, not its tests)
from test_surface_restatement_cpu import MAX_UNDECIDED_SHARE, ORACLE_MAX_CUM_DIFF, QS, dyadic_rays  # noqa: E402

pytestmark = pytest.mark.gpu

H = 1e-3
DTYPES = ["f32", "bf16", "bf16x3", "f16x2"]
Q8 = np.float32([0.25, 0.5, 0.75, 1.0, 0.125, 0.3, 0.9, 1e-3])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- 1. the stage calls -------------------------------------------------------------------------------------------------------------------
def synthetic_weights(n_rays, n):
    """Dyadic weights (every partial sum exact: the quantiles of Q8 that are multiples of 1/8 are hit as exact ties), rays that add up
    to exactly 1, an all-zero ray, rays of ordinary (inexact) weights and rays with a NaN weight."""
    rng = np.random.default_rng(1000 * n_rays + n)
    w, t, _ = dyadic_rays(rng, n_rays, n)
    for r in range(n_rays):
        kind = r % 6
        if kind == 1:                                                  # the sum is exactly 1 (q = 1 is reached on the last non-zero sample)
            w[r] = 0.0
            w[r, rng.integers(0, n, min(n, 4))] = 0.25
            w[r, rng.integers(0, n)] += np.float32(1.0) - w[r].sum(dtype=np.float32)
        elif kind == 2:
            w[r] = (rng.uniform(0, 1, n) ** 4 / n * 3).astype(np.float32)
        elif kind == 3 and n > 1:
            w[r, rng.integers(0, n)] = np.nan
        elif kind == 4:
            w[r] = 0.0
    return w, t


@pytest.mark.parametrize("n", [1, 8, 16, 17, 70, 512])
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 130])
def test_stage_ray_quantiles_is_its_restatement(renderer, n_rays, n):
    w, t = synthetic_weights(n_rays, n)
    for n_q in (1, 3, 8):
        qs = Q8[:n_q]
        want, index = SR.quantile_depths(w, t, qs, return_index=True)
        got = renderer.stage_ray_quantiles(w, t, qs)
        assert got.shape == (n_q, n_rays) and got.dtype == np.float32
        assert _same(got, want), (n_q, np.flatnonzero((_bits(got) != _bits(want)).any(axis=0))[:8])
    if n_rays >= 63 and n >= 8:
        assert (index >= 0).any() and (index < 0).any()               # both outcomes occur
        j_idx, r_idx = np.nonzero(index >= 0)
        assert (SR.cumulative(w)[r_idx, index[j_idx, r_idx]] == Q8[j_idx]).any()      # an exact tie cum_i == q is among the crossings


def gather_inputs(n_rays, pattern, per_ray):
    rng = np.random.default_rng(7 * n_rays + len(pattern))
    o = rng.normal(size=(n_rays, 3)).astype(np.float32) if per_ray else np.float32([0.5, -0.25, 4.0])
    d = rng.normal(size=(n_rays, 3)).astype(np.float32)
    dq = rng.uniform(2.0, 6.0, n_rays).astype(np.float32)
    A = rng.uniform(0.5, 1.0, n_rays).astype(np.float32)
    if pattern == "third":
        dq[::3] = 0.0                                                  # no crossing
        A[1::7] = np.float32(0.25)                                     # too transparent
        A[4::50] = np.float32(0.5)                                     # exactly on the threshold: kept
        A[5::61] = np.nan
    elif pattern == "none":
        dq[:] = 0.0
    C_ = (rng.uniform(0, 1, (n_rays, 3)).astype(np.float32) * A[:, None]).astype(np.float32)
    nrm = rng.normal(size=(n_rays, 3)).astype(np.float32)
    return o, d, dq, C_, A, nrm


def check_records(got, want, normals, cap=None):
    m = want["n"] if cap is None else min(want["n"], cap)
    assert got["n_points"] == want["n"]
    assert np.array_equal(got["ray"][:m], want["ray"][:m])
    for k in ("xyz", "rgb", "depth", "opacity") + (("normals",) if normals else ()):
        assert _same(got[k][:m], want[k][:m]), k
    for k, v in got.items():                                           # nothing behind the records, nothing behind the capacity
        if k in ("xyz", "rgb", "depth", "opacity", "normals"):
            assert (_bits(v[m:]) == 0xFFFFFFFF).all(), k
        elif k == "ray":
            assert (v[m:] == 0xFFFFFFFF).all()
    for k, g in got["guards"].items():
        assert (g == 0xFFFFFFFF).all(), k


@pytest.mark.parametrize("per_ray", [False, True], ids=["shared", "per-ray"])
@pytest.mark.parametrize("n_rays", [1, 255, 256, 257, 1000])
def test_stage_gather_points_is_its_restatement(renderer, n_rays, per_ray):
    for pattern in ("third", "none", "all"):
        o, d, dq, C_, A, nrm = gather_inputs(n_rays, pattern, per_ray)
        want = SR.points(o, d, dq, C_, A, nrm, 0.5)
        assert want["n"] == (0 if pattern == "none" else n_rays if pattern == "all" else want["n"])
        got = renderer.stage_gather_points(o, d, dq, C_, A, nrm, 0.5)
        assert not got["overflow"]
        check_records(got, want, True)
        if want["n"] > 0:                                              # a capacity one short: the first capacity points, the full count, the error
            short = renderer.stage_gather_points(o, d, dq, C_, A, None, 0.5, capacity=want["n"] - 1)
            assert short["overflow"] and "normals" not in short
            check_records(short, want, False, cap=want["n"] - 1)
    if n_rays == 1000:
        o, d, dq, C_, A, nrm = gather_inputs(n_rays, "third", per_ray)
        assert 500 < SR.points(o, d, dq, C_, A, nrm, 0.5)["n"] < 700
        for a in (0.0, 1.0):
            check_records(renderer.stage_gather_points(o, d, dq, C_, A, nrm, a), SR.points(o, d, dq, C_, A, nrm, a), True)


def test_stage_gather_overflow_is_a_state_error(native, renderer):
    o, d, dq, C_, A, nrm = gather_inputs(300, "all", True)
    from nerf_rs_amd import _lib
    cnt = __import__("ctypes").c_size_t(0)
    bufs = [np.zeros(3 * 299 + 64, np.float32) for _ in range(2)]
    p = lambda v: v.ctypes.data_as(_lib.f32p)  # noqa: E731
    rc = renderer._L.nerf_stage_gather_points(renderer.handle, 300, p(o), 300, p(d), p(dq), p(C_), p(A), None, 0.5, 299, p(bufs[0]), p(bufs[1]), None, None, None,
                                              None, __import__("ctypes").byref(cnt))
    msg = renderer._L.nerf_last_error(renderer.handle).decode()
    assert rc == -6 and cnt.value == 300 and "300" in msg and "299" in msg, (rc, msg)


# ---- 2. render_rays(quantiles=...) ----------------------------------------------------------------------------------------------------------
def _render(native, r, origins, dirs, near, far, nf, qs=QS, **kw):
    """(rgb, depth, opacity, depth_q) of the call with quantiles, after checking that the first three are the bits of the call without."""
    kw.setdefault("normalize", False)
    got = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, quantiles=qs, **kw)
    plain = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, **kw)
    assert len(got) == 4 and got[3].shape == (len(qs), len(dirs)) and got[3].dtype == np.float32
    for k in range(3):
        assert _same(got[k], plain[k]), ("colour, depth, opacity must not notice the quantiles", k)
    return got


@pytest.fixture(scope="module")
def ragged(native, renderer, samples):
    """130 lego rays (a 13 x 10 window) with displaced origins and bounds cycling through three (near, far) pairs; restated once per case."""
    be = RR.GpuBackend(native, renderer)
    cam = native.camera_from_samples(samples, 800, 800, 20)
    origins, dirs, bounds = RB.displaced_batch(be, cam, (311, 286, 13, 10))
    origins = np.vstack([origins, be.geometry(cam)[1][None, :]])     # row 130: the camera's own origin, the shared-origin cases'
    cache = {}

    def case(nc, nf, shared=False, coarse_only=False, dtype="f32", background=None):
        key = (nc, nf, shared, coarse_only, dtype, background)
        if key not in cache:
            o = origins[130] if shared else origins[:130]
            rs = RB.restate_rays(be, o, dirs, 0.0, 0.0, bounds, None, nc, nf, 11, coarse_only, dtype, background=background)
            rs["depth_q"] = SR.quantile_depths(rs["w_fine"], rs["t_fine"], QS)
            for a in rs.values():
                a.setflags(write=False)
            cache[key] = rs
        return cache[key]

    origins.setflags(write=False)
    return origins, dirs, bounds, case


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nc,nf", [(3, 5), (7, 10), (20, 50)])
def test_quantile_depths_are_their_restatement(native, renderer, ragged, nc, nf, n):
    origins, dirs, bounds, case = ragged
    kw = dict(n_coarse=nc, bounds=bounds[:n], seed=11)
    rs = case(nc, nf)
    got = _render(native, renderer, origins[:n], dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(got[0], rs["rgb"][:n]) and _same(got[2], rs["opacity"][:n])
    assert _same(got[3], rs["depth_q"][:, :n]), np.abs(got[3] - rs["depth_q"][:, :n]).max()
    if n == 130 and nc == 20:
        reached = rs["depth_q"][1] != 0
        assert reached.sum() >= 8 and (~reached).sum() >= 8            # rays through the model and rays that meet nothing, both
    # one origin for every ray: ray-mode launches; the same origin repeated: points-mode launches -- the same bits
    rs = case(nc, nf, shared=True)
    shared = _render(native, renderer, origins[130], dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(shared[3], rs["depth_q"][:, :n])
    repeated = _render(native, renderer, np.tile(origins[130], (n, 1)), dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(repeated[3], shared[3])


def test_coarse_only_and_no_fine_samples_walk_the_coarse_samples(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 0, coarse_only=True)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 0, n_coarse=20, bounds=bounds, seed=11, coarse_only=True)
    assert _same(got[0], rs["rgb"]) and _same(got[3], rs["depth_q"])
    rs = case(20, 0)                                                   # n_fine = 0: the fine network on the coarse samples
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 0, n_coarse=20, bounds=bounds, seed=11)
    assert _same(got[0], rs["rgb"]) and _same(got[3], rs["depth_q"]) and (rs["depth_q"][1] != 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_come_from_the_renders_arithmetic(native, renderer, ragged, dtype):
    origins, dirs, bounds, case = ragged
    rs = case(20, 50, dtype=dtype)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11, dtype=dtype)
    assert _same(got[0], rs["rgb"]) and _same(got[3], rs["depth_q"])
    if dtype == "bf16":
        assert not _same(rs["w_fine"], case(20, 50)["w_fine"])        # another arithmetic, other weights


def test_eight_quantiles_and_their_order(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 50)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, qs=Q8, n_coarse=20, bounds=bounds, seed=11)
    assert _same(got[3], SR.quantile_depths(rs["w_fine"], rs["t_fine"], Q8))
    assert _same(got[3][:3], rs["depth_q"])


def test_rays_that_meet_nothing(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    away = _render(native, renderer, origins[130], -dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11)
    assert (away[2] == 0).all() and (_bits(away[3]) == 0).all()


@pytest.mark.parametrize("cap", [13, 50])
def test_passes_that_end_inside_the_batch(native, renderer, ragged, monkeypatch, cap):
    """NERF_MAX_RAYS_PER_PASS (read when a context is created): 117 rays in 9 passes of 13 and in passes of 50, 50 and 17.  The quantile
    planes are n_rays apart whatever the pass size; the point cloud's running offset crosses every pass boundary."""
    origins, dirs, bounds, case = ragged
    n = 117
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(cap))
    with native.Renderer(0) as r2:
        r2.load_scene(SCENE)
        for shared in (False, True):
            rs = case(20, 50, shared=shared)
            o = origins[130] if shared else origins[:n]
            got = native.render_rays(r2.coarse, r2.fine, o, dirs[:n], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[:n], seed=11, normalize=False, aux=True,
                                     quantiles=QS, return_stats=True)
            assert got[4].n_passes == -(-n // cap)
            assert _same(got[0], rs["rgb"][:n]) and _same(got[3], rs["depth_q"][:, :n])
        for h in (None, H):
            want = _cloud_from_renders(native, renderer, origins[:n], dirs[:n], bounds[:n], 0.5, 0.5, h)
            cloud, st = native.point_cloud(r2.coarse, r2.fine, origins[:n], dirs[:n], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[:n], seed=11, normalize=False,
                                           normals_h=h, return_stats=True)
            assert st.n_passes == -(-n // cap)
            _check_cloud(cloud, want, h is not None)
            assert want["n"] >= 20 and len(set((want["ray"] // cap).tolist())) >= 3      # kept rays in at least three passes


# ---- 3. invariants ---------------------------------------------------------------------------------------------------------------------------
def test_depth_q_implies_opacity_and_is_monotone(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    qs = np.float32([0.05, 0.25, 0.5, 0.75, 0.95, 1.0])
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, qs=qs, n_coarse=20, bounds=bounds, seed=11)
    opacity, dq = got[2], got[3]
    for j, q in enumerate(qs):
        assert (opacity[dq[j] != 0] >= q).all() and (dq[j][opacity >= q] != 0).all(), q
        assert ((dq[j] >= bounds[:, 0]) & (dq[j] <= bounds[:, 1]))[dq[j] != 0].all()
    for j in range(1, len(qs)):
        both = dq[j] != 0
        assert (dq[j - 1][both] != 0).all() and (dq[j - 1][both] <= dq[j][both]).all()
    assert (dq[0] < dq[4])[dq[4] != 0].any()


def test_permuting_a_batch_permutes_its_quantile_depths(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 50)
    perm = np.random.default_rng(7).permutation(len(dirs))
    idx = np.arange(len(dirs), dtype=np.uint32)
    got = _render(native, renderer, origins[:130][perm], dirs[perm], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[perm], rng_index=idx[perm], seed=11)
    assert _same(got[3], rs["depth_q"][:, perm])
    assert len(set(_bits(rs["depth_q"][1]).tolist())) > 40             # the depths differ: an ignored permutation would show


def test_device_forms_agree_with_the_host_forms(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    n = 130
    rs = case(20, 50)
    want_cloud = _cloud_from_renders(native, renderer, origins[:n], dirs, bounds, 0.5, 0.5, H)
    device = DeviceBuffers(native)
    try:
        d_o, d_d, d_b = device.upload(origins[:n]), device.upload(dirs), device.upload(bounds)
        d_rgb, d_op, d_dq = device.upload(np.zeros((n, 3), np.float32)), device.upload(np.zeros(n, np.float32)), device.upload(np.full((3, n), -7.0, np.float32))
        native.render_rays_device(renderer.coarse, renderer.fine, d_o, n, d_d, n, 0.0, 0.0, 50, d_rgb, n_coarse=20, d_bounds=d_b, normalize=False, seed=11,
                                  d_opacity=d_op, d_depth_q=d_dq, quantiles=QS)
        assert _same(device.download(d_dq, (3, n), np.float32), rs["depth_q"]) and _same(device.download(d_rgb, (n, 3), np.float32), rs["rgb"])
        # the point cloud into guarded device arrays: capacity n, then one short of the count
        for cap in (n, want_cloud["n"] - 1):
            guard = np.full(8, np.float32(-7.0))
            d_xyz, d_c, d_n = (device.upload(np.full(3 * cap + 8, -7.0, np.float32)) for _ in range(3))
            d_ray, d_dep, d_a = device.upload(np.full(cap + 8, 0xABABABAB, np.uint32)), device.upload(np.full(cap + 8, -7.0, np.float32)), device.upload(np.full(cap + 8, -7.0, np.float32))
            d_cnt = device.upload(np.uint32([0xFFFFFFFF]))
            kw = dict(normals_h=H, d_normals=d_n, d_ray=d_ray, d_depth=d_dep, d_opacity=d_a, d_n_points=d_cnt, n_coarse=20, d_bounds=d_b, normalize=False, seed=11)
            if cap == n:
                count = native.point_cloud_device(renderer.coarse, renderer.fine, d_o, n, d_d, n, 0.0, 0.0, 50, cap, d_xyz, d_c, want_count=True, **kw)
                assert count == want_cloud["n"]
            else:
                with pytest.raises(native.NerfError) as e:
                    native.point_cloud_device(renderer.coarse, renderer.fine, d_o, n, d_d, n, 0.0, 0.0, 50, cap, d_xyz, d_c, want_count=True, **kw)
                assert e.value.code == -6 and str(want_cloud["n"]) in e.value.msg and str(cap) in e.value.msg
            assert int(device.download(d_cnt, (1,), np.uint32)[0]) == want_cloud["n"]
            m = min(cap, want_cloud["n"])
            for ptr, key, width in ((d_xyz, "xyz", 3), (d_c, "rgb", 3), (d_n, "normals", 3), (d_dep, "depth", 1), (d_a, "opacity", 1)):
                back = device.download(ptr, (width * cap + 8,), np.float32)
                assert _same(back[:width * m], want_cloud[key][:m].reshape(-1)), key
                assert _same(back[width * m:], np.full(width * (cap - m) + 8, -7.0, np.float32)), key      # nothing behind the records or the capacity
            back = device.download(d_ray, (cap + 8,), np.uint32)
            assert np.array_equal(back[:m], want_cloud["ray"][:m]) and (back[m:] == 0xABABABAB).all()
            del guard
    finally:
        device.close()


def test_device_entry_points_on_torch_tensors():
    """tests/helpers/surface_torch_child.py: torch tensors in and out on a torch stream -- render_rays_device(d_depth_q=, quantiles=) in f32
    and f16x2, point_cloud_device without and with normals, with and without the host count, per-ray and shared origins, three passes --
    the bits of the host entry points.  A process of its own (torch's HIP runtime must load first)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "surface_torch_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok 52", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def test_image_renders_do_not_notice(native, renderer, samples, ragged):
    origins, dirs, bounds, _ = ragged
    cam = native.camera_from_samples(samples, 800, 800, 64)
    crop = (311, 287, 13, 9)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11)
    native.point_cloud(renderer.coarse, renderer.fine, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11, normalize=False, normals_h=H)
    after = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    for k in range(3):
        assert _same(after[k], before[k])


# ---- 4. point clouds -----------------------------------------------------------------------------------------------------------------------
def _cloud_from_renders(native, r, origins, dirs, bounds, quantile, min_opacity, h, nc=20, nf=50, dtype="f32", coarse_only=False):
    """The helper fed with the per-ray outputs of render_rays over a black background (quantile depth included) and of
    render_rays(normals_h=h)."""
    kw = dict(n_coarse=nc, bounds=bounds, seed=11, normalize=False, dtype=dtype, coarse_only=coarse_only, background=(0.0, 0.0, 0.0), aux=True)
    C_, _, A, dq = native.render_rays(r.coarse, r.fine, origins, dirs, 0.0, 0.0, nf, quantiles=[quantile], **kw)
    normals = None if h is None else native.render_rays(r.coarse, r.fine, origins, dirs, 0.0, 0.0, nf, normals_h=h, **kw)[3]
    return SR.points(origins, dirs, dq[0], C_, A, normals, min_opacity)


def _check_cloud(cloud, want, normals):
    assert len(cloud["ray"]) == want["n"] and cloud["ray"].dtype == np.uint32
    assert np.array_equal(cloud["ray"], want["ray"]) and (np.diff(cloud["ray"].astype(np.int64)) > 0).all()
    for k in ("xyz", "rgb", "depth", "opacity") + (("normals",) if normals else ()):
        assert cloud[k].dtype == np.float32 and _same(cloud[k], want[k]), k
    assert ("normals" in cloud) == normals


@pytest.mark.parametrize("h", [None, H], ids=["plain", "normals"])
@pytest.mark.parametrize("min_opacity", [0.0, 0.5, 1.0])
def test_point_cloud_is_its_restatement(native, renderer, ragged, min_opacity, h):
    origins, dirs, bounds, case = ragged
    want = _cloud_from_renders(native, renderer, origins[:130], dirs, bounds, 0.5, min_opacity, h)
    rs = case(20, 50, background=(0.0, 0.0, 0.0))
    base = SR.points(origins[:130], dirs, rs["depth_q"][1], rs["rgb"], rs["opacity"], None, min_opacity)      # and from the stage calls alone
    assert np.array_equal(base["ray"], want["ray"]) and _same(base["xyz"], want["xyz"]) and _same(base["rgb"], want["rgb"])
    cloud = native.point_cloud(renderer.coarse, renderer.fine, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11, normalize=False,
                               min_opacity=min_opacity, normals_h=h)
    _check_cloud(cloud, want, h is not None)
    if min_opacity == 0.5:
        assert 20 <= want["n"] < 130 and np.isfinite(cloud["rgb"]).all()
        if h is not None:
            assert (np.abs(cloud["normals"]).sum(axis=1) > 0).sum() >= 8
    shared = native.point_cloud(renderer.coarse, renderer.fine, origins[130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11, normalize=False,
                                min_opacity=min_opacity, normals_h=h)
    _check_cloud(shared, _cloud_from_renders(native, renderer, origins[130], dirs, bounds, 0.5, min_opacity, h), h is not None)


@pytest.mark.parametrize("shared", [False, True], ids=["per-ray", "shared"])
def test_point_cloud_of_unnormalised_directions(native, oracle, renderer, ragged, shared):
    """normalize=True on scaled directions: the points lie along d, the direction the networks saw -- Vec3::normalize of the input, which
    the helper is fed from the oracle's normalize (DESIGN section 2 records it as the device's, bit for bit) --, not along the input."""
    origins, dirs, bounds, _ = ragged
    scale = np.random.default_rng(3).uniform(0.25, 4.0, len(dirs)).astype(np.float32)
    scaled = (dirs * scale[:, None]).astype(np.float32)
    unit = np.stack([oracle.normalize(v) for v in scaled])
    assert not _same(unit, dirs) and not _same(unit, scaled)          # neither the unit directions of the other tests nor the input
    o = origins[130] if shared else origins[:130]
    kw = dict(n_coarse=20, bounds=bounds, seed=11, normalize=True)
    C_, _, A, dq = native.render_rays(renderer.coarse, renderer.fine, o, scaled, 0.0, 0.0, 50, background=(0.0, 0.0, 0.0), aux=True, quantiles=[0.5], **kw)
    normals = native.render_rays(renderer.coarse, renderer.fine, o, scaled, 0.0, 0.0, 50, normals_h=H, **kw)[1]
    want = SR.points(o, unit, dq[0], C_, A, normals, 0.5)
    cloud = native.point_cloud(renderer.coarse, renderer.fine, o, scaled, 0.0, 0.0, 50, normals_h=H, **kw)
    _check_cloud(cloud, want, True)
    along_input = SR.points(o, scaled, dq[0], C_, A, normals, 0.5)
    assert want["n"] >= 20 and not _same(along_input["xyz"], want["xyz"])


@pytest.mark.parametrize("quantile,dtype,coarse_only", [(0.25, "f32", False), (0.9, "f16x2", False), (0.5, "f32", True), (1.0, "bf16", False)])
def test_point_cloud_other_quantiles_and_arithmetics(native, renderer, ragged, quantile, dtype, coarse_only):
    origins, dirs, bounds, _ = ragged
    nf = 0 if coarse_only else 50
    want = _cloud_from_renders(native, renderer, origins[:130], dirs, bounds, quantile, 0.3, None, nf=nf, dtype=dtype, coarse_only=coarse_only)
    cloud = native.point_cloud(renderer.coarse, renderer.fine, origins[:130], dirs, 0.0, 0.0, nf, n_coarse=20, bounds=bounds, seed=11, normalize=False,
                               quantile=quantile, min_opacity=0.3, dtype=dtype, coarse_only=coarse_only)
    _check_cloud(cloud, want, False)


def test_point_cloud_capacity_and_empty_batches(native, renderer, ragged):
    origins, dirs, bounds, _ = ragged
    want = _cloud_from_renders(native, renderer, origins[:130], dirs, bounds, 0.5, 0.5, None)
    kw = dict(n_coarse=20, bounds=bounds, seed=11, normalize=False)
    exact = native.point_cloud(renderer.coarse, renderer.fine, origins[:130], dirs, 0.0, 0.0, 50, capacity=want["n"], **kw)
    _check_cloud(exact, want, False)
    with pytest.raises(native.NerfError) as e:
        native.point_cloud(renderer.coarse, renderer.fine, origins[:130], dirs, 0.0, 0.0, 50, capacity=want["n"] - 1, **kw)
    assert e.value.code == -6 and str(want["n"]) in e.value.msg and str(want["n"] - 1) in e.value.msg
    empty = native.point_cloud(renderer.coarse, renderer.fine, origins[130], np.zeros((0, 3), np.float32), 2.0, 6.0, 50, n_coarse=20)
    assert empty["xyz"].shape == (0, 3) and empty["ray"].shape == (0,)
    away = native.point_cloud(renderer.coarse, renderer.fine, origins[130], -dirs, 0.0, 0.0, 50, **kw)
    assert away["xyz"].shape == (0, 3)


def test_render_image_points_carries_the_cameras_batch(native, renderer, samples):
    cam = native.camera_from_samples(samples, 96, 96, 20)
    crop = (19, 55, 7, 5)
    be = RR.GpuBackend(native, renderer)
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, crop)
    want = native.point_cloud(renderer.coarse, renderer.fine, origin, dirs, near, far, 50, n_coarse=20, rng_index=pix, seed=5, normalize=False, normals_h=H)
    got = native.render_image_points(renderer.coarse, renderer.fine, cam, 50, normals_h=H, seed=5, crop=crop)
    _check_cloud(got, dict(want, n=len(want["ray"])), True)
    assert len(got["ray"]) > 0 and (got["ray"] < 35).all()
    image = native.render_image(renderer.coarse, renderer.fine, cam, 50, seed=5, crop=crop, aux=True)
    assert _same(got["opacity"], image[2].reshape(-1)[got["ray"]])     # the opacities are the image render's


def _ply_vertex_block(native, cloud):
    cols = [np.ascontiguousarray(cloud["xyz"], "<f4").view(np.uint8).reshape(-1, 12)]
    if "normals" in cloud:
        cols.append(np.ascontiguousarray(cloud["normals"], "<f4").view(np.uint8).reshape(-1, 12))
    cols.append(native.quantize_rgb8(cloud["rgb"]).reshape(-1, 3))
    return np.hstack(cols).tobytes()


def test_cli_points_and_median_depth_are_the_librarys(native, renderer, samples, tmp_path):
    """nerf_cli --points FILE.ply: a PLY with zero faces whose vertex block is the bytes of point_cloud -- of the --rays batch, and of the
    camera's rays; --depth-quantile FILE.pfm: the median depth of the window through the PFM writer."""
    rng = np.random.default_rng(5)
    n = 65
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
    d = (rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32) - o).astype(np.float32)
    np.hstack([o, d]).astype("<f4").tofile(tmp_path / "rays.f32")
    exe = os.path.join(os.path.dirname(native.lib_path()), "nerf_cli")
    common = ["--scene", SCENE, "--coarse", "20", "--fine", "50", "--seed", "9"]
    p = subprocess.run([exe, "--rays", str(tmp_path / "rays.f32"), "--points", str(tmp_path / "p.ply"), "--points-quantile", "0.5", "--points-min-opacity", "0.4",
                        "--normals-step", "0.002"] + common, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0, (p.stdout, p.stderr)
    want = native.point_cloud(renderer.coarse, renderer.fine, o, d, float(samples["near"]), float(samples["far"]), 50, n_coarse=20, seed=9, min_opacity=0.4,
                              normals_h=0.002)
    raw = (tmp_path / "p.ply").read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert len(want["ray"]) >= 5 and f"element vertex {len(want['ray'])}\n".encode() in raw[:end] and b"element face 0\n" in raw[:end]
    assert raw[end:] == _ply_vertex_block(native, want)
    assert not (tmp_path / "output.ppm").exists()                    # no image flag: no render
    # the camera's rays, without normals, and the median-depth map of the same window
    p = subprocess.run([exe, "--width", "96", "--height", "96", "--crop", "19,55,7,5", "--points", str(tmp_path / "c.ply"), "--depth-quantile", str(tmp_path / "m.pfm"),
                        "--out", str(tmp_path / "c.ppm"), "--scene", SCENE, "--coarse", "20", "--fine", "50", "--seed", "5"], capture_output=True, text=True,
                       timeout=120, cwd=tmp_path)
    assert p.returncode == 0, (p.stdout, p.stderr)
    cam = native.camera_from_samples(samples, 96, 96, 20)
    cloud = native.render_image_points(renderer.coarse, renderer.fine, cam, 50, seed=5, crop=(19, 55, 7, 5))
    raw = (tmp_path / "c.ply").read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert len(cloud["ray"]) > 0 and raw[end:] == _ply_vertex_block(native, cloud) and b"property float nx" not in raw[:end]
    be = RR.GpuBackend(native, renderer)
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, (19, 55, 7, 5))
    median = native.render_rays(renderer.coarse, renderer.fine, origin, dirs, near, far, 50, n_coarse=20, rng_index=pix, seed=5, normalize=False, quantiles=[0.5])[1]
    native.save_pfm(tmp_path / "want.pfm", 7, 5, median[0])
    assert (tmp_path / "m.pfm").read_bytes() == (tmp_path / "want.pfm").read_bytes()
    p = subprocess.run([exe, "--rays", str(tmp_path / "rays.f32"), "--points", str(tmp_path / "p.ply"), "--points-quantile", "0"] + common, capture_output=True,
                       text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 1 and "a quantile must be finite and lie in (0, 1]" in p.stderr


# ---- 5. the oracle -------------------------------------------------------------------------------------------------------------------------
def test_quantile_depths_against_the_oracle(native, oracle, oracle_nets, renderer, samples):
    """The GPU's quantile depths on the window of tests/test_normal_restatement_cpu.py against the ORACLE's weights.  D, the largest
    difference between the partial sums of the two back ends of restate_rays over all samples of the window, is measured here and
    compared with the recorded ORACLE_MAX_CUM_DIFF (at twice the figure: card-to-card variation).  A ray is decided for q when no oracle
    cum_i lies within 2 D of q: the GPU's crossing is then the oracle's sample or a neighbour of it."""
    P = LEGO_NORMALS
    obe, gbe = RR.OracleBackend(oracle, *oracle_nets), RR.GpuBackend(native, renderer)
    ocam = oracle.camera_from_samples(samples, P["W"], P["W"])
    origin, dirs, near, far, pix = RB.camera_batch(obe, ocam, P["crop"])
    ors = RB.restate_rays(obe, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    grs = RB.restate_rays(gbe, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    ocum, gcum = SR.cumulative(ors["w_fine"]), SR.cumulative(grs["w_fine"])
    D = float(np.abs(gcum.astype(np.float64) - ocum.astype(np.float64)).max())
    print(f"\nlargest |cum_gpu - cum_oracle| over {ocum.size} samples: D = {D:.3e}; largest |t_gpu - t_oracle| = {np.abs(grs['t_fine'] - ors['t_fine']).max():.3e}")
    assert ORACLE_MAX_CUM_DIFF is not None, f"measured D = {D:.3e}: record it in tests/test_surface_restatement_cpu.py"
    assert D <= 2.0 * ORACLE_MAX_CUM_DIFF, (D, ORACLE_MAX_CUM_DIFF)
    cam = native.camera_from_samples(samples, P["W"], P["W"], P["nc"])
    _, gdirs, _, _, gpix = RB.camera_batch(gbe, cam, P["crop"])
    got = native.render_rays(renderer.coarse, renderer.fine, np.float32(list(cam.pos)), gdirs, near, far, P["nf"], n_coarse=P["nc"], rng_index=gpix,
                             seed=P["seed"], normalize=False, quantiles=QS)[1]
    _, oindex = SR.quantile_depths(ors["w_fine"], ors["t_fine"], QS, return_index=True)
    n = ors["t_fine"].shape[1]
    for j, q in enumerate(QS):
        reach = ors["opacity"] >= np.float32(q)
        near_q = (np.abs(ocum.astype(np.float64) - float(np.float32(q))) <= 2.0 * ORACLE_MAX_CUM_DIFF).any(axis=1)
        decided = reach & ~near_q
        share = float((reach & near_q).sum()) / max(int(reach.sum()), 1)
        print(f"q = {q}: {int(decided.sum())} of {int(reach.sum())} rays decided ({share:.3f} undecided)")
        assert reach.sum() >= 100 and share <= MAX_UNDECIDED_SHARE
        k = oindex[j][decided]
        rows = np.flatnonzero(decided)
        lo, hi = ors["t_fine"][rows, np.maximum(k - 1, 0)], ors["t_fine"][rows, np.minimum(k + 1, n - 1)]
        assert ((got[j][decided] >= lo) & (got[j][decided] <= hi)).all(), (q, rows[(got[j][decided] < lo) | (got[j][decided] > hi)])
