"""The premises of the zero-step-skip GPU tests, proved without a GPU from the oracle and float64 (tests/helpers/zero_skip_cases.py):
every engineered network does to its points what its case says, and the float64 bracket of the executed ReLU k-steps is tight on every
(network, batch) pair whose counters test_gpu_zero_skip_kernels.py brackets -- at most 0.1 % of the k-steps uncertain, at least 1 % certainly
dead, so that neither "skips nothing" nor "skips something live" fits inside it."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import write_random_net

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import zero_skip_cases as Z  # noqa: E402


@pytest.fixture(scope="module")
def random_net(tmp_path_factory):
    return write_random_net(tmp_path_factory.mktemp("zskip_cpu") / "net", 20240)


@pytest.fixture(scope="module")
def cases(oracle, random_net, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("zskip_cpu_cases")
    return {c: Z._make_case(c, random_net, tmp, oracle) for c in Z.CASES}


def test_step_units_are_the_layout():
    """Every hidden unit is read by exactly one k-step, two units per step, sixteen steps per 32-unit tile."""
    assert sorted(Z.STEP_UNITS.reshape(-1)) == list(range(256))
    assert all(set(Z.STEP_UNITS[16 * t:16 * t + 16].reshape(-1)) == set(range(32 * t, 32 * t + 32)) for t in range(8))
    assert tuple(Z.STEP_UNITS[3]) == (3, 7)                         # the register test_gpu_zero_skip.py's dead_register_net kills


def test_bracket_on_a_made_up_layer():
    z = np.full((40, 256), -1.0)                                    # 40 points -> one workgroup tile, 4 waves (the last point repeated)
    z[0, 3] = 1.0                                                   # wave 0, step 3 (units 3, 7): live
    z[33, 7] = 5e-4                                                 # wave 1, step 3: neither above +eps nor all below -eps
    z[39, 200] = 1.0                                                # the last point: wave 1 and, as padding, waves 2 and 3
    live, dead, total = Z.kstep_bracket([z])
    assert total == 4 * 128 and live == 1 + 3 and dead == total - live - 1
    assert Z.n_waves(1) == 4 and Z.n_waves(128) == 4 and Z.n_waves(129) == 8 and Z.n_waves(315) == 12


@pytest.mark.parametrize("case", Z.CASES)
def test_engineered_condition_holds(oracle, cases, case):
    d, twin = cases[case]
    pts, dirs, live = Z.case_points(case)
    ergb, esg = Z.check_case(case, oracle, d, twin, pts, dirs, live)
    pre = Z.preacts_fp64(d, pts)
    if case == "b":                                                 # ... and from float64: dense3's outputs feed dense4 nothing
        assert pre[3].max() < -100
    if case == "e":
        assert pre[6].max() < -100 and np.array_equal(pre[7], np.tile(Z.subnormal_bias().astype(np.float64), (Z.N_MAX, 1)))
        b = Z.subnormal_bias()
        assert np.all(np.abs(b[8:]) >= 1e-41) and np.all(np.abs(b) < 1.1754944e-38) and (b > 0).sum() > 64 and (b < 0).sum() > 64
        print(f"\ncase e: sigma {esg[0]:.7f} (float64 {Z.subnormal_sigma_fp64():.7f}), rgb std {ergb.std():.3f}")
    if case in "cf":                                                # h0 = x on every unit, exactly
        assert np.array_equal(pre[0], np.tile(pts[0].astype(np.float64)[:, None], (1, 256)))
        assert Z.dead_wave_steps(live) == 128 * 64                  # half of the 128 waves


def test_poisoned_batch():
    pts, dirs, hit = Z.poisoned_points()
    clean = Z.uniform_points()[0]
    differ = (pts.view(np.uint32) != clean.view(np.uint32)).sum(axis=0)
    assert hit.sum() == 10 and np.array_equal(differ, hit.astype(int)) and hit[-1]
    assert Z.POISON_AT[0] // 32 == Z.POISON_AT[1] // 32 and len(set(Z.POISON_AT // 32)) == 9
    assert np.isnan(pts).sum() == 2 and np.isinf(pts).sum() == 2
    assert sorted(pts.view(np.uint32)[np.arange(10) % 3, Z.POISON_AT]) == sorted(Z.POISON.view(np.uint32))
    assert sorted(np.signbit(pts[np.isnan(pts)]).tolist()) == [False, True]


def test_ray_batch_is_ray_ordered():
    pts, dirs = Z.ray_points()
    assert pts.shape == (3, Z.N_MAX) and dirs.shape == (Z.N_MAX, 3)
    p = pts.T.reshape(128, 32, 3)
    step = np.diff(p, axis=1)                                       # one ray per wave: equally spaced along its direction
    assert np.abs(step - step[:, :1]).max() < 1e-5 and np.allclose(np.linalg.norm(dirs, axis=1), 1, atol=1e-6)
    assert np.array_equal(dirs.reshape(128, 32, 3)[:, 0], dirs.reshape(128, 32, 3)[:, 31])


BATCHES = {"rays": Z.ray_points, "uniform": lambda: Z.uniform_points()}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("net", ("coarse", "fine", "random"))
def test_bracket_is_tight(random_net, net, batch):
    d = random_net if net == "random" else os.path.join(SCENE, net)
    pre = Z.preacts_fp64(d, BATCHES[batch]()[0])
    for layers in (8, 7):                                           # forward_batch, density()
        live, dead, total = Z.kstep_bracket(pre[:layers])
        print(f"\n{net} {batch} {layers} layers: certainly live {live}, certainly dead {dead} ({100 * dead / total:.2f} %), uncertain {total - live - dead} of {total}")
        assert total == 128 * layers * 128
        assert total - live - dead <= 1e-3 * total
        assert dead >= 0.01 * total


def test_case_f_window_sees_both_half_spaces(oracle, samples, cases):
    """The render window of case f in the GPU file: some of its rays stay in x < 0 from near to far (sigma exactly 0 on all of their
    samples: whole tiles without density, rays without a live sample), others reach x > 0 and meet density there."""
    x0, y0, w, h = Z.F_WINDOW
    cam = oracle.camera_from_samples(samples, 800, 800)
    o = np.float32(samples["camera_origin"])
    d = np.stack([oracle.normalize(oracle.get_ray_dir(cam, y0 + i, x0 + j)) for i in range(h) for j in range(w)])
    t = np.linspace(samples["near"], samples["far"], 32, dtype=np.float32)
    p = (o[None, None, :] + d[:, None, :] * t[None, :, None]).astype(np.float32)
    empty = (p[..., 0] < 0).all(axis=1)
    _, sg = oracle.Net(cases["f"][0]).forward_batch(np.ascontiguousarray(p.reshape(-1, 3).T), np.repeat(d, 32, axis=0))
    dense = (sg.reshape(-1, 32) > 0).any(axis=1)
    print(f"\n{Z.F_WINDOW}: {int(empty.sum())} of {empty.size} rays stay in x < 0; {int(dense.sum())} rays meet density")
    assert empty.sum() >= 0.1 * empty.size and dense.sum() >= 0.25 * empty.size and not dense[empty].any()
    assert empty.reshape(h, w)[:, -11:].all()                       # eleven whole rays in a row: 11 x 192 fine samples, whole 128-point tiles among them
