"""Surface normals on the GPU (nerf_density_gradient_batch, nerf_render_rays_normals; contract: include/nerf_mi355x.h, "surface normals"):
every output is compared BIT FOR BIT with tests/helpers/normal_restatement.py run on Network.density of the same context and on the
positions and weights tests/helpers/ray_batch_restatement.py restates from the stage calls.

  1. density_gradient: n = 1, 63, 65, 130, 1000 points, h = 1e-3 and 1e-2, both networks, host and device entry points, a zero
     denominator, a forced small internal chunk;
  2. render_rays(normals_h=...): 1 .. 130 lego rays at 3 + 5 and 20 + 50 samples with per-ray origins and three (near, far) pairs, a shared
     origin, coarse_only, all four arithmetics (weights in the render's arithmetic, gradients in f32), rays that meet nothing, passes that
     end inside the batch;
  3. the invariants: colour, depth and opacity keep their bits; a permutation permutes; render_image_normals carries render_image's
     colour; image renders do not notice; torch tensors; the command-line tool;
  4. the GPU's normals against the oracle-backed restatement of tests/test_normal_restatement_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import normal_restatement as NR  # noqa: E402
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402
from test_gpu_density import DeviceBuffers  # noqa: E402  (the helper, not its tests)
from test_normal_restatement_cpu import LEGO_NORMALS, oracle_density  # noqa: E402  (the window and the oracle's density, not its tests)

pytestmark = pytest.mark.gpu

H = 1e-3
DTYPES = ["f32", "bf16", "bf16x3", "f16x2"]
# largest angle (degrees) between the GPU's normal and the oracle-backed restated normal over the rays of LEGO_NORMALS with opacity > 0.5,
# measured on an MI355X: see test_normals_against_the_oracle.  The test asserts twice this figure.
ORACLE_MAX_ANGLE_DEG = 0.0283


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _density(net):
    return lambda pts: net.density(np.ascontiguousarray(pts, np.float32))


def _render(native, r, origins, dirs, near, far, nf, h=H, **kw):
    """(rgb, depth, opacity, normals) of the call with normals, after checking that the first three are the bits of the call without."""
    kw.setdefault("normalize", False)
    got = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, normals_h=h, **kw)
    plain = native.render_rays(r.coarse, r.fine, origins, dirs, near, far, nf, aux=True, **kw)
    assert len(got) == 4 and got[3].shape == (len(dirs), 3) and got[3].dtype == np.float32
    for k in range(3):
        assert _same(got[k], plain[k]), ("colour, depth, opacity must not notice the normals", k)
    return got


def _restated_normals(r, rs, origins, coarse_only=False, h=H, n=None):
    net = r.coarse if coarse_only else r.fine
    n = len(rs["dirs"]) if n is None else n
    o = origins if np.ndim(origins) == 1 else origins[:n]
    return NR.ray_normals(_density(net), o, rs["dirs"][:n], rs["t_fine"][:n], rs["w_fine"][:n], h)


# ---- 1. density_gradient ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_points():
    return np.random.default_rng(31).uniform(-1.2, 1.2, (3, 1000)).astype(np.float32)       # the lego box


@pytest.mark.parametrize("name", ["coarse", "fine"])
@pytest.mark.parametrize("h", [1e-3, 1e-2])
@pytest.mark.parametrize("n", [1, 63, 65, 130, 1000])
def test_density_gradient_is_its_restatement(native, renderer, box_points, n, h, name):
    net = renderer.coarse if name == "coarse" else renderer.fine
    pts = np.ascontiguousarray(box_points[:, :n])
    want = NR.gradient(_density(net), pts, h)
    got = net.density_gradient(pts, h)
    assert got.shape == (3, n) and got.dtype == np.float32
    assert _same(got, want), np.abs(got - want).max()
    if n == 1000:
        assert (np.abs(want).max(axis=0) > 0).mean() > 0.05 and np.isfinite(want).all()       # the box holds the model: not all zero
    device = DeviceBuffers(native)
    try:
        d_pts, d_grad = device.upload(pts), device.upload(np.full((3, n), -7.0, np.float32))
        net.density_gradient_device(d_pts, d_grad, n, h)
        assert _same(device.download(d_grad, (3, n), np.float32), want)
    finally:
        device.close()


def test_density_gradient_edges(renderer):
    assert renderer.fine.density_gradient(np.zeros((3, 0), np.float32), H).shape == (3, 0)
    p = np.float32([[100.0, 0.1], [0.0, 0.2], [-100.0, 0.3]])                 # |p| = 100, h = 1e-7: p +- h == p, the denominator is 0
    g = renderer.fine.density_gradient(p, 1e-7)
    assert (_bits(g[[0, 2], 0]) == 0).all()
    assert _same(g, NR.gradient(_density(renderer.fine), p, 1e-7))


@pytest.mark.parametrize("chunk", [1, 64, 333])
def test_density_gradient_does_not_notice_its_chunks(native, renderer, box_points, monkeypatch, chunk):
    """NERF_GRADIENT_CHUNK (read when a context is created): 1000 points in chunks of 1, 64 and 333 -- the last one ragged."""
    want = renderer.fine.density_gradient(box_points, H)
    monkeypatch.setenv("NERF_GRADIENT_CHUNK", str(chunk))
    n = 130 if chunk == 1 else 1000
    with native.Renderer(0) as r2:
        r2.load_scene(SCENE)
        assert _same(r2.fine.density_gradient(np.ascontiguousarray(box_points[:, :n]), H), want[:, :n])


# ---- 2. render_rays(normals_h=...) ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(native, renderer, samples):
    """130 lego rays (a 13 x 10 window) with displaced origins and bounds cycling through three (near, far) pairs; restated once per case
    (per-ray origins at two sample shapes, one shared origin, coarse_only, the four arithmetics) together with the restated normals."""
    be = RR.GpuBackend(native, renderer)
    cam = native.camera_from_samples(samples, 800, 800, 20)
    origins, dirs, bounds = RB.displaced_batch(be, cam, (311, 286, 13, 10))
    origins = np.vstack([origins, be.geometry(cam)[1][None, :]])     # row 130: the camera's own origin, the shared-origin cases'
    cache = {}

    def case(nc, nf, shared=False, coarse_only=False, dtype="f32"):
        key = (nc, nf, shared, coarse_only, dtype)
        if key not in cache:
            o = origins[130] if shared else origins[:130]
            rs = RB.restate_rays(be, o, dirs, 0.0, 0.0, bounds, None, nc, nf, 11, coarse_only, dtype)
            rs["normals"] = _restated_normals(renderer, rs, o, coarse_only)
            for a in rs.values():
                a.setflags(write=False)
            cache[key] = rs
        return cache[key]

    origins.setflags(write=False)
    return origins, dirs, bounds, case


@pytest.mark.parametrize("n", [1, 63, 65, 117, 130])
@pytest.mark.parametrize("nc,nf", [(3, 5), (20, 50)])
def test_ray_normals_are_their_restatement(native, renderer, ragged, nc, nf, n):
    origins, dirs, bounds, case = ragged
    kw = dict(n_coarse=nc, bounds=bounds[:n], seed=11)
    rs = case(nc, nf)
    if (nc, nf, n) == (20, 50, 130):
        assert NR.live_count(rs["w_fine"]) > 256                      # the live list spans several 256-entry scan blocks
    got = _render(native, renderer, origins[:n], dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(got[0], rs["rgb"][:n])
    assert _same(got[3], rs["normals"][:n]), np.abs(got[3] - rs["normals"][:n]).max()
    if n == 130:
        hit = rs["opacity"] > 0.5
        assert hit.any() and (rs["opacity"] == 0).any()               # rays through the model and rays that meet nothing, both
        assert np.allclose((got[3][hit].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6) and (got[3][rs["opacity"] == 0] == 0).all()
    # one origin for every ray: ray-mode launches; the same origin repeated: points-mode launches -- the same bits
    rs = case(nc, nf, shared=True)
    shared = _render(native, renderer, origins[130], dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(shared[3], rs["normals"][:n])
    repeated = _render(native, renderer, np.tile(origins[130], (n, 1)), dirs[:n], 0.0, 0.0, nf, **kw)
    assert _same(repeated[3], shared[3])
    if n == 130:
        assert (np.abs(shared[3]).sum(axis=1) > 0).sum() >= 8


def test_coarse_only_differentiates_the_coarse_network(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 0, coarse_only=True)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 0, n_coarse=20, bounds=bounds, seed=11, coarse_only=True)
    assert _same(got[0], rs["rgb"]) and _same(got[3], rs["normals"])
    fine = NR.ray_normals(_density(renderer.fine), origins[:130], rs["dirs"], rs["t_fine"], rs["w_fine"], H)
    assert not _same(fine, rs["normals"])                             # the other network would show


@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_come_from_the_renders_arithmetic(native, renderer, ragged, dtype):
    """The weights are nerf_stage_integrate's on the render's own sigma (restated in `dtype`); the gradients are f32 whatever dtype is."""
    origins, dirs, bounds, case = ragged
    rs = case(20, 50, dtype=dtype)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11, dtype=dtype)
    assert _same(got[0], rs["rgb"]) and _same(got[3], rs["normals"]), np.abs(got[3] - rs["normals"]).max()
    if dtype == "bf16":
        assert not _same(rs["w_fine"], case(20, 50)["w_fine"])        # another arithmetic, other weights


def test_another_step(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 50)
    want = _restated_normals(renderer, rs, origins[:130], h=1e-2)
    got = _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, h=1e-2, n_coarse=20, bounds=bounds, seed=11)
    assert _same(got[3], want) and not _same(want, rs["normals"])


def test_rays_that_meet_nothing(native, renderer, ragged):
    """A batch aimed away from the scene has no live sample: zero normals (+0, every bit), nothing is evaluated.  Mixed with live rays
    (every second ray that carries a normal, and every second that does not, is turned away) each ray keeps the bits it has on its own."""
    origins, dirs, bounds, case = ragged
    rs = case(20, 50, shared=True)
    kw = dict(n_coarse=20, bounds=bounds, seed=11)
    away = _render(native, renderer, origins[130], -dirs, 0.0, 0.0, 50, **kw)
    assert (away[2] == 0).all() and (_bits(away[3]) == 0).all()
    mixed_dirs = dirs.copy()
    flipped = np.zeros(len(dirs), bool)
    carries = np.abs(rs["normals"]).sum(axis=1) > 0
    assert carries.sum() >= 8
    flipped[np.flatnonzero(carries)[::2]] = True; flipped[np.flatnonzero(~carries)[::2]] = True     # every second ray of either kind
    mixed_dirs[flipped] = -dirs[flipped]
    got = _render(native, renderer, origins[130], mixed_dirs, 0.0, 0.0, 50, **kw)
    assert (_bits(got[3][flipped]) == 0).all()
    assert _same(got[3][~flipped], rs["normals"][~flipped]) and (np.abs(got[3][~flipped]).sum(axis=1) > 0).any()


@pytest.mark.parametrize("cap", [13, 50])
def test_passes_that_end_inside_the_batch(native, renderer, ragged, monkeypatch, cap):
    """NERF_MAX_RAYS_PER_PASS (read when a context is created): 117 rays in 9 passes of 13 and in passes of 50, 50 and 17 -- every pass
    re-bases its rays, its live list and its outputs; one of the passes of 13 may hold no live sample at all."""
    origins, dirs, bounds, case = ragged
    n = 117
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(cap))
    with native.Renderer(0) as r2:
        r2.load_scene(SCENE)
        for shared in (False, True):
            rs = case(20, 50, shared=shared)
            o = origins[130] if shared else origins[:n]
            got = native.render_rays(r2.coarse, r2.fine, o, dirs[:n], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[:n], seed=11, normalize=False, aux=True,
                                     normals_h=H, return_stats=True)
            assert got[4].n_passes == -(-n // cap)
            assert _same(got[0], rs["rgb"][:n]) and _same(got[3], rs["normals"][:n])
        rs = case(20, 50, dtype="f16x2")
        got = native.render_rays(r2.coarse, r2.fine, origins[:n], dirs[:n], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[:n], seed=11, normalize=False,
                                 dtype="f16x2", normals_h=H)
        assert _same(got[1], rs["normals"][:n])


# ---- 3. invariants ---------------------------------------------------------------------------------------------------------------------------
def test_permuting_a_batch_permutes_its_normals(native, renderer, ragged):
    origins, dirs, bounds, case = ragged
    rs = case(20, 50)
    perm = np.random.default_rng(7).permutation(len(dirs))
    idx = np.arange(len(dirs), dtype=np.uint32)
    got = _render(native, renderer, origins[:130][perm], dirs[perm], 0.0, 0.0, 50, n_coarse=20, bounds=bounds[perm], rng_index=idx[perm], seed=11)
    assert _same(got[3], rs["normals"][perm])
    assert len({tuple(v) for v in _bits(rs["normals"]).tolist()}) > 40          # the normals differ: an ignored permutation would show


def test_render_image_normals_carries_the_image_render(native, renderer, samples):
    cam = native.camera_from_samples(samples, 96, 96, 20)
    crop = (19, 55, 7, 5)
    want = native.render_image(renderer.coarse, renderer.fine, cam, 50, seed=5, crop=crop, aux=True)
    got = native.render_image_normals(renderer.coarse, renderer.fine, cam, 50, h=H, seed=5, crop=crop)
    assert got[0].shape == (5, 7, 3) and got[3].shape == (5, 7, 3)
    for k in range(3):
        assert _same(got[k], want[k]), k
    assert not (want[0] == 1.0).all()
    be = RR.GpuBackend(native, renderer)
    rs = RR.restate(be, cam, 20, 50, crop, 5)
    normals = NR.ray_normals(_density(renderer.fine), cam.pos, rs["dirs"], rs["t_fine"], rs["w_fine"], H)
    assert _same(got[3].reshape(-1, 3), normals)
    full = native.render_image_normals(renderer.coarse, renderer.fine, native.camera_from_samples(samples, 12, 12, 20), 50, h=H, seed=5)
    assert full[0].shape == (12, 12, 3) and full[3].shape == (12, 12, 3)


def test_image_renders_do_not_notice_a_normals_call(native, renderer, samples, ragged):
    origins, dirs, bounds, _ = ragged
    cam = native.camera_from_samples(samples, 800, 800, 64)
    crop = (311, 287, 13, 9)
    renderer.kernel_time_query(reset=True)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    _render(native, renderer, origins[:130], dirs, 0.0, 0.0, 50, n_coarse=20, bounds=bounds, seed=11)
    renderer.fine.density_gradient(np.zeros((3, 5), np.float32), H)
    _, points, launches = renderer.kernel_time_query(reset=False)
    assert launches == 1 and points == 13 * 9 * 192                    # the sigma launches of the normals are not the dominant kernel
    after = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=3, crop=crop, aux=True)
    for k in range(3):
        assert _same(after[k], before[k])
    renderer.kernel_time_query(reset=True)


def test_device_entry_points_on_torch_tensors():
    """tests/helpers/normals_torch_child.py: torch tensors in and out on a torch stream, per-ray and shared origins, f32 and f16x2, and
    density_gradient_device -- the bits of the host entry points.  A process of its own (torch's HIP runtime must load first)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "normals_torch_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok 17", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def test_cli_rays_normals_are_the_librarys(native, renderer, samples, tmp_path):
    """nerf_cli --rays FILE --rays-out FILE --rays-normals FILE --normals-step H: n x 3 f32 normals, the bytes of render_rays(normals_h=H)."""
    rng = np.random.default_rng(5)
    n = 65
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
    d = (rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32) - o).astype(np.float32)
    np.hstack([o, d]).astype("<f4").tofile(tmp_path / "rays.f32")
    cli = [os.path.join(os.path.dirname(native.lib_path()), "nerf_cli"), "--scene", SCENE, "--rays", str(tmp_path / "rays.f32"), "--rays-out", str(tmp_path / "rgb.f32"),
           "--coarse", "20", "--fine", "50", "--seed", "9"]
    p = subprocess.run(cli + ["--rays-normals", str(tmp_path / "n.f32"), "--normals-step", "0.002"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0, (p.stdout, p.stderr)
    want = native.render_rays(renderer.coarse, renderer.fine, o, d, float(samples["near"]), float(samples["far"]), 50, n_coarse=20, seed=9, normals_h=0.002)
    assert (tmp_path / "n.f32").read_bytes() == np.ascontiguousarray(want[1]).astype("<f4").tobytes()
    assert (tmp_path / "rgb.f32").read_bytes() == np.ascontiguousarray(want[0]).astype("<f4").tobytes()
    assert (np.abs(want[1]).sum(axis=1) > 0).any()
    p = subprocess.run(cli + ["--rays-normals", str(tmp_path / "n.f32"), "--normals-step", "0"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 1 and "must be finite and greater than 0" in p.stderr
    # the image run's normal map: 0.5 n + 0.5 through the PPM quantiser
    p = subprocess.run([cli[0], "--scene", SCENE, "--width", "96", "--height", "96", "--crop", "19,55,7,5", "--coarse", "20", "--fine", "50", "--seed", "5",
                        "--out", str(tmp_path / "c.ppm"), "--normals", str(tmp_path / "n.ppm")], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0, (p.stdout, p.stderr)
    cam = native.camera_from_samples(samples, 96, 96, 20)
    maps = native.render_image_normals(renderer.coarse, renderer.fine, cam, 50, h=1e-3, seed=5, crop=(19, 55, 7, 5))
    enc = (np.float32(0.5) * maps[3] + np.float32(0.5)).astype(np.float32)
    assert (tmp_path / "n.ppm").read_bytes() == b"P6\n7 5\n255\n" + native.quantize_rgb8(enc).tobytes()
    assert (tmp_path / "c.ppm").read_bytes() == b"P6\n7 5\n255\n" + native.quantize_rgb8(maps[0]).tobytes()


# ---- 4. the oracle -------------------------------------------------------------------------------------------------------------------------
def test_normals_against_the_oracle(native, oracle, oracle_nets, renderer, samples):
    """The GPU's normals on the window of tests/test_normal_restatement_cpu.py against the restatement on the ORACLE's networks and samples.
    Differencing divides the difference between the two f32 evaluations of sigma by 2 h = 2e-3; what that leaves of the agreement is
    measured here (ORACLE_MAX_ANGLE_DEG, recorded in DESIGN 4.14) and asserted at twice the measured value, over the rays both sides see
    with opacity > 0.5.  The GPU's own normals must also face the camera on 90 % of those rays."""
    P = LEGO_NORMALS
    be = RR.OracleBackend(oracle, *oracle_nets)
    ocam = oracle.camera_from_samples(samples, P["W"], P["W"])
    origin, dirs, near, far, pix = RB.camera_batch(be, ocam, P["crop"])
    rs = RB.restate_rays(be, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    want = NR.ray_normals(oracle_density(oracle_nets[1]), origin, rs["dirs"], rs["t_fine"], rs["w_fine"], P["h"])
    cam = native.camera_from_samples(samples, P["W"], P["W"], P["nc"])
    rgb, depth, opacity, got = native.render_image_normals(renderer.coarse, renderer.fine, cam, P["nf"], h=P["h"], seed=P["seed"], crop=P["crop"])
    got, opacity = got.reshape(-1, 3), opacity.reshape(-1)
    hit = (opacity > 0.5) & (rs["opacity"] > 0.5)
    assert hit.sum() >= 100
    ang = NR.angle_deg(got[hit], want[hit])
    facing = ((got * rs["dirs"]).sum(axis=1) < 0)[opacity > 0.5]
    print(f"\nGPU normals vs the oracle-backed restatement, {int(hit.sum())} rays: largest angle {ang.max():.4f} deg, median {np.median(ang):.5f} deg; "
          f"{int(facing.sum())} of {facing.size} GPU normals face the camera ({facing.mean():.3f})")
    assert facing.mean() >= 0.90, facing.mean()
    assert ORACLE_MAX_ANGLE_DEG is not None, f"measured {ang.max():.4f} deg: record it"
    assert ang.max() <= 2.0 * ORACLE_MAX_ANGLE_DEG, (ang.max(), ORACLE_MAX_ANGLE_DEG)
