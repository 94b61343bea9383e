"""Ray clipping on the device (nerf_occupancy_dilate, nerf_clip_rays, nerf_render_rays_clipped and their _device forms; -m gpu).  Every
equality is bit for bit (floats compared as uint32).

  1. nerf_clip_rays and nerf_clip_rays_device == tests/helpers/ray_clip.py (checked against a float64 brute force on the CPU:
     tests/test_ray_clip_cpu.py) on the CPU test's rays, for the grids 13 x 9 x 11, 33 x 2 x 1, 1 x 1 x 1 and 40^3 with a 2-cell shell;
     one shared origin == that origin repeated per ray; n_hit == the sum of the flags;
  2. nerf_occupancy_dilate[_device] == the restatement on the same dims with r = 1, 2, 4, with n_occupied and bounds;
  3. render_rays_clipped on a 24 x 24 lego camera's rays behind the fine network's 32^3 occupancy (threshold 1, dilate 1) ==
     render_rays on the hit rays alone with bounds = the clip's and rng_index = the original indices, scattered over background / 0 / 0:
     three sample plans, per-ray origins, a caller rng_index, another background, normalize=False; a permuted batch gives permuted
     outputs; the all-empty grid returns the background everywhere with n_hit = 0; the _device entry on torch tensors (a child process);
     nerf_cli --rays-occupancy [--occupancy-dilate]."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_clip as RC  # noqa: E402
from test_gpu_density import DeviceBuffers  # noqa: E402  (the helper, not its tests)

pytestmark = pytest.mark.gpu

F = np.float32
GRIDS = {
    "13x9x11": ((13, 9, 11), (0.21, 0.19, 0.17), lambda: RC.random_grid((13, 9, 11), 0.06, seed=3)),
    "33x2x1": ((33, 2, 1), (0.21, 0.19, 0.17), lambda: RC.random_grid((33, 2, 1), 0.2, seed=5)),
    "1x1x1": ((1, 1, 1), (0.21, 0.19, 0.17), lambda: np.uint32([1])),
    "40x40x40 shell": ((40, 40, 40), (0.06, 0.06, 0.06), RC.shell_grid),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the clip ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_clip_rays_is_the_restatement(native, renderer, name):
    dims, step, make = GRIDS[name]
    bits, lo = make(), RC.GRID_LO
    rays = RC.make_rays(lo, step, dims)                                     # for 13 x 9 x 11 the CPU test's 3000 rays; all finite
    o, d, b = rays["origins"], rays["dirs"], rays["bounds"]
    assert np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(b).all()
    want, want_hit = RC.clip_rays(bits, lo, step, dims, o, d, 0.0, 0.0, bounds=b)
    assert 0 < want_hit.sum() < want_hit.size
    out, hit, count = native.clip_rays(renderer, bits, lo, step, dims, o, d, 0.0, 0.0, bounds=b, return_count=True)
    assert count == int(hit.sum()) == int(want_hit.sum())
    assert np.array_equal(hit, want_hit) and np.array_equal(_bits(out), _bits(want))
    # one origin for every ray == that origin repeated; one [near, far] for every ray; directions as they are
    for normalize in (True, False):
        w2, h2 = RC.clip_rays(bits, lo, step, dims, o[11], d, 0.5, 4.0, normalize=normalize)
        shared = native.clip_rays(renderer, bits, lo, step, dims, o[11], d, 0.5, 4.0, normalize=normalize, return_count=True)
        repeated = native.clip_rays(renderer, bits, lo, step, dims, np.tile(o[11], (len(d), 1)), d, 0.5, 4.0, normalize=normalize)
        assert np.array_equal(shared[1], h2) and np.array_equal(_bits(shared[0]), _bits(w2)) and shared[2] == int(h2.sum())
        assert np.array_equal(repeated[1], h2) and np.array_equal(_bits(repeated[0]), _bits(w2))
    # the device entry point: per-ray and shared origins, with and without the count
    n = len(d)
    dev = DeviceBuffers(native)
    try:
        d_bits, d_o, d_d, d_b = dev.upload(bits), dev.upload(o), dev.upload(d), dev.upload(b)
        d_out, d_hit = dev.upload(np.full((n + 1, 2), -7.5, F)), dev.upload(np.full(n + 1, 9, np.uint8))
        got = native.clip_rays_device(renderer, d_bits, lo, step, dims, d_o, n, d_d, n, 0.0, 0.0, d_out, d_hit, d_bounds=d_b, want_count=True)
        out, hit = dev.download(d_out, (n + 1, 2), F), dev.download(d_hit, (n + 1,), np.uint8)
        assert got == int(want_hit.sum()) and np.array_equal(hit[:n], want_hit) and np.array_equal(_bits(out[:n]), _bits(want))
        assert (out[n] == F(-7.5)).all() and hit[n] == 9                      # nothing behind the last ray is written
        w2, h2 = RC.clip_rays(bits, lo, step, dims, o[11], d, 0.5, 4.0)
        d_o1 = dev.upload(o[11])
        assert native.clip_rays_device(renderer, d_bits, lo, step, dims, d_o1, 1, d_d, n, 0.5, 4.0, d_out, d_hit) is None
        out, hit = dev.download(d_out, (n + 1, 2), F), dev.download(d_hit, (n + 1,), np.uint8)
        assert np.array_equal(hit[:n], h2) and np.array_equal(_bits(out[:n]), _bits(w2))
    finally:
        dev.close()


# ---- 2. dilation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_dilation_is_the_restatement(native, renderer, name):
    dims, _, make = GRIDS[name]
    bits = make() if name != "40x40x40 shell" else RC.random_grid(dims, 0.002, seed=8)
    n_words = len(bits)
    dev = DeviceBuffers(native)
    try:
        d_in = dev.upload(bits)
        for radius in (1, 2, 4):
            want, count, bounds = RC.dilate(bits, dims, radius)
            got = native.dilate_occupancy(renderer, bits, dims, radius, return_stats=True)
            assert np.array_equal(got[0], want) and got[1:] == (count, bounds), (name, radius)
            assert np.array_equal(native.dilate_occupancy(renderer, bits, dims, radius), want)
            d_out = dev.upload(np.full(n_words + 1, 0xDEADBEEF, np.uint32))
            assert native.dilate_occupancy_device(renderer, d_in, dims, radius, d_out, want_stats=True) == (count, bounds)
            out = dev.download(d_out, (n_words + 1,), np.uint32)
            assert np.array_equal(out[:n_words], want) and out[n_words] == 0xDEADBEEF
    finally:
        dev.close()


# ---- 3. the clipped render -----------------------------------------------------------------------------------------------------------------
LEGO_LO, LEGO_DIMS = (-1.3, -1.3, -0.8), (32, 32, 32)
LEGO_STEP = (2.6 / 32, 2.6 / 32, 2.2 / 32)
KEYS = ("rgb", "depth", "opacity")


@pytest.fixture(scope="module")
def lego(native, renderer, samples):
    """The grid and the rays of item 3: the fine network's 32^3 occupancy over README's lego box at threshold 1, dilated by 1; a 24 x 24
    camera's rays (unit directions), their clip, computed once."""
    _, bits, count, _ = renderer.fine.density_grid(LEGO_LO, LEGO_STEP, LEGO_DIMS, threshold=1.0, want_sigma=False)
    grown = native.dilate_occupancy(renderer, bits, LEGO_DIMS, 1)
    cam = native.camera_from_samples(samples, 24, 24, 16)
    dirs = renderer.stage_ray_dirs(cam, 0, 0, 24, 24, normalize=True).reshape(-1, 3)
    clip, hit = native.clip_rays(renderer, grown, LEGO_LO, LEGO_STEP, LEGO_DIMS, cam.pos, dirs, cam.near, cam.far, normalize=False)
    assert 0 < count < 32 ** 3 and 40 < hit.sum() < 500                    # the model fills a part of the frame
    return dict(bits=grown, cam=cam, dirs=dirs, clip=clip, hit=hit)


def _expected(native, r, origins, dirs, clip, hit, index, background, **kw):
    """render_rays on the hit rays alone with the clip's bounds and their own indices, scattered over background / 0 / 0"""
    n = len(dirs)
    o = origins if np.ndim(origins) == 1 else origins[hit]
    rgb = np.tile(np.float32([1, 1, 1] if background is None else background), (n, 1))
    depth, opacity = np.zeros(n, F), np.zeros(n, F)
    if hit.any():
        got = native.render_rays(r.coarse, r.fine, o, dirs[hit], 0.0, 0.0, bounds=clip[hit], rng_index=index[hit], background=background, aux=True, **kw)
        rgb[hit], depth[hit], opacity[hit] = got
    return rgb, depth, opacity


def _same(got, want, what):
    for k, g, w in zip(KEYS, got, want):
        bad = _bits(g) != _bits(w)
        assert not bad.any(), f"{what} {k}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


PLANS = {"16+24": dict(n_coarse=16, fine_samples_per_ray=24), "coarse_only": dict(n_coarse=16, fine_samples_per_ray=24, coarse_only=True),
         "16+0": dict(n_coarse=16, fine_samples_per_ray=0)}


@pytest.mark.parametrize("plan", list(PLANS))
def test_clipped_render_is_render_rays_on_the_hit_rays(native, renderer, lego, plan):
    kw = dict(PLANS[plan], seed=4)
    cam, dirs, clip, hit = lego["cam"], lego["dirs"], lego["clip"], lego["hit"]
    n = len(dirs)
    grid = (lego["bits"], LEGO_LO, LEGO_STEP, LEGO_DIMS)
    arange = np.arange(n, dtype=np.uint32)
    got = native.render_rays_clipped(renderer.coarse, renderer.fine, *grid, cam.pos, dirs, cam.near, cam.far, normalize=False, aux=True,
                                     return_hit=True, return_stats=True, **kw)
    assert np.array_equal(got[3], hit) and got[4] == int(hit.sum()) and got[5].n_rays == int(hit.sum())
    want = _expected(native, renderer, cam.pos, dirs, clip, hit, arange, None, normalize=False, **kw)
    _same(got[:3], want, plan)
    assert (got[2][hit] > 0).any() and not (got[0][hit] == 1).all()        # the model is in the picture
    if plan != "16+24":
        return
    # colour alone
    assert np.array_equal(_bits(native.render_rays_clipped(renderer.coarse, renderer.fine, *grid, cam.pos, dirs, cam.near, cam.far, normalize=False, **kw)),
                          _bits(want[0]))
    # per-ray origins (the points-mode launches), a caller rng_index, another background, directions normalised on the device
    origins = np.tile(cam.pos, (n, 1))
    origins[::3] += np.float32([0.05, -0.03, 0.02])
    raw = (dirs * np.linspace(0.5, 3.0, n, dtype=F)[:, None]).astype(F)
    index = (arange * 5 + 3).astype(np.uint32)
    bg = (0.25, 0.5, 0.125)
    clip2, hit2 = native.clip_rays(renderer, *grid, origins, raw, cam.near, cam.far)
    got = native.render_rays_clipped(renderer.coarse, renderer.fine, *grid, origins, raw, cam.near, cam.far, rng_index=index, background=bg, aux=True,
                                     return_hit=True, **kw)
    assert np.array_equal(got[3], hit2) and 0 < hit2.sum() < n
    want2 = _expected(native, renderer, origins, raw, clip2, hit2, index, bg, **kw)
    _same(got[:3], want2, "per-ray origins")
    assert (got[0][~hit2] == np.float32(bg)).all() and (got[1][~hit2] == 0).all() and (got[2][~hit2] == 0).all()
    # the caller's own per-ray bounds in front of the clip
    own = np.stack([np.full(n, cam.near, F), np.linspace(cam.near + 0.5, cam.far, n, dtype=F)], axis=1)
    clip3, hit3 = native.clip_rays(renderer, *grid, origins, raw, 0.0, 0.0, bounds=own)
    got3 = native.render_rays_clipped(renderer.coarse, renderer.fine, *grid, origins, raw, 0.0, 0.0, bounds=own, rng_index=index, aux=True, return_hit=True, **kw)
    assert np.array_equal(got3[3], hit3) and 0 < hit3.sum() <= hit2.sum() and not np.array_equal(_bits(clip3), _bits(clip2))
    _same(got3[:3], _expected(native, renderer, origins, raw, clip3, hit3, index, None, **kw), "own bounds")
    # a permuted batch (rng_index along with it) gives permuted outputs
    perm = np.random.default_rng(1).permutation(n)
    gp = native.render_rays_clipped(renderer.coarse, renderer.fine, *grid, origins[perm], raw[perm], cam.near, cam.far, rng_index=index[perm],
                                    background=bg, aux=True, **kw)
    _same(gp, [w[perm] for w in want2], "permuted")
    # the all-empty grid: the background everywhere, nothing hit, nothing rendered
    empty = np.zeros_like(lego["bits"])
    ge = native.render_rays_clipped(renderer.coarse, renderer.fine, empty, LEGO_LO, LEGO_STEP, LEGO_DIMS, origins, raw, cam.near, cam.far, background=bg,
                                    aux=True, return_hit=True, return_stats=True, **kw)
    assert (ge[0] == np.float32(bg)).all() and (ge[1] == 0).all() and (ge[2] == 0).all() and not ge[3].any() and ge[4] == 0
    assert ge[5].n_rays == 0 and ge[5].n_mlp_launches == 0


def test_device_entry_point_on_torch_tensors():
    """tests/helpers/ray_clip_torch_child.py: torch tensors in and out on a torch stream -- the bits of the host entry points.  A process of
    its own, because it must load torch's HIP runtime before the library's (see tests/helpers/ray_batch_torch_child.py)."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "ray_clip_torch_child.py")
    p = subprocess.run([sys.executable, child, SCENE], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok 14", (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def test_cli_rays_occupancy(native, renderer, samples, lego, tmp_path):
    """nerf_cli --rays ... --rays-occupancy FILE --density-grid / --grid-lo / --grid-step [--occupancy-dilate R]: the words --grid-occupancy
    writes go back in, the rays are clipped (nerf_render_rays_clipped) and no grid or image is produced beside them."""
    cam, dirs = lego["cam"], lego["dirs"]
    n = len(dirs)
    np.hstack([np.tile(cam.pos, (n, 1)), dirs]).astype("<f4").tofile(tmp_path / "rays.f32")
    exe = os.path.join(os.path.dirname(native.lib_path()), "nerf_cli")
    lattice = ["--density-grid", "32,32,32", "--grid-lo", "-1.3,-1.3,-0.8", "--grid-step", f"{2.6 / 32!r},{2.6 / 32!r},{2.2 / 32!r}"]
    p = subprocess.run([exe, "--scene", SCENE] + lattice + ["--grid-threshold", "1", "--grid-occupancy", str(tmp_path / "occ.bits")], capture_output=True,
                       text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0, (p.stdout, p.stderr)
    raw = np.fromfile(tmp_path / "occ.bits", "<u4")
    assert np.array_equal(native.dilate_occupancy(renderer, raw, LEGO_DIMS, 1), lego["bits"])
    cli = [exe, "--scene", SCENE, "--rays", str(tmp_path / "rays.f32"), "--rays-out", str(tmp_path / "rgb.f32"), "--rays-occupancy", str(tmp_path / "occ.bits")] + lattice
    p = subprocess.run(cli + ["--occupancy-dilate", "1", "--coarse", "16", "--fine", "24", "--seed", "4"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    want, _, hits = native.render_rays_clipped(renderer.coarse, renderer.fine, lego["bits"], LEGO_LO, LEGO_STEP, LEGO_DIMS, cam.pos, dirs, float(samples["near"]),
                                               float(samples["far"]), 24, n_coarse=16, seed=4, return_hit=True)     # the CLI normalises on the device
    assert p.returncode == 0 and 0 < hits < n and f"{n} rays, {hits} of them cross an occupied cell (16 coarse + 24 fine samples)" in p.stdout, (p.stdout, p.stderr)
    assert not (tmp_path / "output.ppm").exists() and "density grid" not in p.stdout
    got = np.fromfile(tmp_path / "rgb.f32", "<f4").reshape(n, 3)
    assert np.array_equal(_bits(got), _bits(want))
    p = subprocess.run(cli + ["--occupancy-dilate", "5"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2                                               # radius outside 1..4: usage
    p = subprocess.run(cli[:-6], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 2                                               # --rays-occupancy without the lattice it belongs to: usage
    (tmp_path / "short.bits").write_bytes(raw.tobytes()[:-4])
    p = subprocess.run(cli[:8] + [str(tmp_path / "short.bits")] + lattice, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 1 and "occupancy words" in p.stderr
