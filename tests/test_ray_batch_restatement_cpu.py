"""tests/helpers/ray_batch_restatement.py checked on the CPU, before the GPU tests of render_rays lean on it (oracle back end):

  * on a camera's rays (origin = the camera's, unit directions, the camera's near / far, rng_index = row * nx + col) the restatement IS
    oracle.render_image, bit for bit, for the eight sample shapes and the three lego windows of tests/test_gpu_render_restatement.py;
  * grouping the rays by their far value for the scalar-far stage calls equals a ray-by-ray loop;
  * depth and opacity summed from the returned weights, and the colour summed over white, are the oracle's own compositing;
  * the batch the GPU test renders with displaced origins and cycling bounds holds white and non-white rays;
  * on the probe scene the mutant (sample 0 of every ray given the previous ray's direction) moves at least 25 % of the rays beyond
    5e-4 -- the figure tests/test_render_restatement_cpu.py asserts for the probe."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402
from test_gpu_render_restatement import LEGO_SEED, LEGO_WINDOWS, SHAPES  # noqa: E402  (the shapes and windows, not its tests)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("nc,nf,coarse_only", SHAPES, ids=[f"{a}+{b}" if not c else f"coarse-only {a}" for a, b, c in SHAPES])
def test_camera_batch_restatement_is_the_oracle_render(oracle, oracle_nets, samples, nc, nf, coarse_only):
    be = RR.OracleBackend(oracle, *oracle_nets)
    white = []
    for W, crop in LEGO_WINDOWS:
        cam = oracle.camera_from_samples(samples, W, W)
        want = oracle.render_image(*oracle_nets, cam, oracle.make_opts(nc, nf, crop=crop, seed=LEGO_SEED, coarse_only=coarse_only))
        origin, dirs, near, far, pix = RB.camera_batch(be, cam, crop)
        got = RB.restate_rays(be, origin, dirs, near, far, None, pix, nc, nf, LEGO_SEED, coarse_only, "f32")
        assert np.array_equal(_bits(got["rgb"]), _bits(want.reshape(-1, 3))), (W, crop)
        n = nc if (coarse_only or nf == 0 or nc < 3) else nc + nf
        assert got["t_fine"].shape == (len(dirs), n) and got["depth"].shape == got["opacity"].shape == (len(dirs),)
        white.append((want == 1.0).all(axis=2).reshape(-1))
    white = np.concatenate(white)
    assert white.any() and not white.all()


def test_unnormalised_directions_and_default_indices(oracle, oracle_nets, samples):
    """normalize=True on raw camera directions gives the unit directions' restatement; rng_index=None is arange."""
    be = RR.OracleBackend(oracle, *oracle_nets)
    cam = oracle.camera_from_samples(samples, 96, 96)
    x0, y0, w, h = 19, 55, 4, 3
    raw = np.stack([oracle.get_ray_dir(cam, y0 + i, x0 + j) for i in range(h) for j in range(w)])
    origin, unit, near, far, _ = RB.camera_batch(be, cam, (x0, y0, w, h))
    assert not np.array_equal(_bits(raw), _bits(unit))
    a = RB.restate_rays(be, origin, raw, near, far, None, None, 20, 50, 5, False, "f32", normalize=True)
    b = RB.restate_rays(be, origin, unit, near, far, None, np.arange(w * h), 20, 50, 5, False, "f32")
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.fixture(scope="module")
def displaced(oracle, oracle_nets, samples):
    D = RB.DISPLACED
    be = RR.OracleBackend(oracle, *oracle_nets)
    cam = oracle.camera_from_samples(samples, D["W"], D["W"])
    origins, dirs, bounds = RB.displaced_batch(be, cam, D["crop"])
    return be, origins, dirs, bounds, RB.restate_rays(be, origins, dirs, 0.0, 0.0, bounds, None, D["nc"], D["nf"], D["seed"], False, "f32")


def test_displaced_batch_holds_white_and_non_white_rays(displaced):
    _, origins, dirs, bounds, rs = displaced
    assert len({tuple(o) for o in origins.tolist()}) == 7 and len({tuple(b) for b in bounds.tolist()}) == 3
    assert (bounds[:, 0] >= 2.0).all() and (bounds[:, 1] <= 6.0).all()
    white = (rs["rgb"] == 1.0).all(axis=1)
    assert white.any() and not white.all(), white.mean()
    assert ((rs["opacity"] == 0.0) == white).all() and (rs["depth"][white] == 0.0).all()
    hit = rs["opacity"] > 0.5
    assert hit.any() and (rs["depth"][hit] / rs["opacity"][hit] > 2.0).all() and (rs["depth"][hit] / rs["opacity"][hit] < 6.0).all()
    for r in range(len(dirs)):        # every ray's samples lie inside its own bounds
        assert bounds[r, 0] <= rs["t_fine"][r].min() and rs["t_fine"][r].max() <= bounds[r, 1]


def test_grouping_by_far_equals_a_ray_by_ray_loop(displaced):
    D = RB.DISPLACED
    be, origins, dirs, bounds, rs = displaced
    one = RB.restate_rays(be, origins, dirs, 0.0, 0.0, bounds, None, D["nc"], D["nf"], D["seed"], False, "f32", group_by_far=False)
    for k in rs:
        assert np.array_equal(_bits(rs[k]), _bits(one[k])), k


def test_depth_opacity_and_background_come_from_the_oracle_weights(oracle, displaced):
    _, _, _, _, rs = displaced
    bg = np.array([0.25, 0.5, -0.125], np.float32)
    rgb, depth, opacity = RB.sums_from_weights(rs["rgb_fine"], rs["w_fine"], rs["t_fine"], bg)
    for r in range(len(depth)):
        w = oracle.compute_weights(rs["sigma_fine"][r], rs["t_fine"][r], float(rs["far"][r]))
        assert np.array_equal(_bits(w), _bits(rs["w_fine"][r]))
        acc = dep = np.float32(0.0)
        c = np.zeros(3, np.float32)
        for i in range(len(w)):
            acc = np.float32(acc + w[i]); dep = np.float32(dep + np.float32(rs["t_fine"][r, i] * w[i]))
            c = (c + rs["rgb_fine"][r, i] * w[i]).astype(np.float32)
        assert _bits(acc) == _bits(opacity[r]) and _bits(dep) == _bits(depth[r]) == _bits(rs["depth"][r])
        assert np.array_equal(_bits(c + bg * np.float32(np.float32(1.0) - acc)), _bits(rgb[r]))


def test_probe_mutant_moves_a_quarter_of_the_rays(oracle, samples, tmp_path):
    P = RR.PROBE
    root = RR.probe_scene(tmp_path / "probe")
    be = RR.OracleBackend(oracle, oracle.Net(str(root / "coarse")), oracle.Net(str(root / "fine")))
    cam = oracle.camera_from_samples(samples, P["size"], P["size"])
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, (0, 0, P["size"], P["size"]))
    args = (be, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    rs, mutant = RB.restate_rays(*args), RB.restate_rays(*args, fine_dirs=RR.roll_first_sample)
    for k in ("t_coarse", "sigma_coarse", "t_fine", "sigma_fine", "w_fine", "depth", "opacity"):
        assert np.array_equal(_bits(rs[k]), _bits(mutant[k])), k
    share = float((np.abs(rs["rgb"] - mutant["rgb"]).max(axis=1) > 5e-4).mean())
    print(f"\nprobe batch, sample 0 misrouted: {share:.3f} of the rays move by more than 5e-4")
    assert share >= 0.25, share
