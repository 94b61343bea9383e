"""The f32 kernels with the bottleneck folded into the viewdirs layer (mlp_kernel.hip, and the colour passes of mlp_kernel_seq.hip),
on the device: forward_batch at sizes that cover a partial wave tile (32 points), a partial workgroup tile (128) and many tiles,
against the live oracle at the existing bounds; and two small windows of the 800x800 view rendered plain, skip_empty, skip_dead and
certify_zero -- the four must be the same bits (the colour passes accumulate in the fused kernel's order) and each must pass Gate 1
against the oracle's render of the window."""
import os

import numpy as np
import pytest

from conftest import SCENE, psnr
from fold_utils import write_random_net

pytestmark = pytest.mark.gpu

N_MAX = 4096
SIZES = (1, 31, 33, 127, 129, N_MAX)


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(77)
    pts = rng.uniform(-2.2, 2.2, size=(3, N_MAX)).astype(np.float32)
    v = rng.normal(size=(N_MAX, 3))
    return pts, (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def random_net(tmp_path_factory):
    return write_random_net(tmp_path_factory.mktemp("fold") / "net", 20240)     # test_fold_host.py's random-weight network


@pytest.fixture(scope="module")
def oracle_outputs(oracle, oracle_nets, random_net, points):
    """The oracle on all 4096 points, once per network; every size below is a prefix (each column is computed alone)."""
    return {"fine": oracle_nets[1].forward_batch(*points), "random": oracle.Net(random_net).forward_batch(*points)}


def _check(rgb, sg, ergb, esg, what):
    ds, dr = np.abs(sg - esg) / (1 + np.abs(esg)), np.abs(rgb - ergb)
    print(f"\n{what}: sigma rel err max {ds.max():.2e}, rgb err max {dr.max():.2e}")
    assert rgb.shape == ergb.shape and sg.shape == esg.shape
    assert np.all(np.abs(sg - esg) <= 1e-4 * (1 + np.abs(esg))) and np.all(dr <= 2e-5)


@pytest.mark.parametrize("n", SIZES)
def test_forward_batch_fine_vs_live_oracle(renderer, points, oracle_outputs, n):
    pts, dirs = points
    rgb, sg = renderer.fine.forward_batch(pts[:, :n], dirs[:n])
    ergb, esg = oracle_outputs["fine"]
    _check(rgb, sg, ergb[:n], esg[:n], f"fine n={n}")


@pytest.mark.parametrize("n", SIZES)
def test_forward_batch_random_net_vs_live_oracle(native, random_net, points, oracle_outputs, n):
    pts, dirs = points
    ergb, esg = oracle_outputs["random"]
    assert (esg > 0).mean() > 0.05 and np.isfinite(esg).all() and ergb.std() > 0.01      # a live network with colours that vary
    with native.Renderer(0) as r:
        net = native.load_network_from_dir(r, 0, random_net)
        rgb, sg = net.forward_batch(pts[:, :n], dirs[:n])
    _check(rgb, sg, ergb[:n], esg[:n], f"random n={n}")


# (x0, y0, w, h) in the 800x800 view: the first lies in the empty background (exactly white: no sample carries weight, every
# colour pass / tile of the colour head has nothing live), the second straddles the model's edge (about a third of its rays hit
# the model; the live samples do not fill the last colour pass)
WINDOWS = {"background 21x13": (3, 5, 21, 13), "edge 48x40": (280, 300, 48, 40)}


@pytest.fixture(scope="module")
def window_refs(oracle, oracle_nets, samples):
    cam = oracle.camera_from_samples(samples, 800, 800)
    return {k: oracle.render_image(oracle_nets[0], oracle_nets[1], cam, oracle.make_opts(64, 128, crop=c, seed=0)) for k, c in WINDOWS.items()}


@pytest.mark.parametrize("window", list(WINDOWS))
def test_window_four_modes_same_bits_and_gate1(renderer, native, samples, window_refs, window):
    crop, ref = WINDOWS[window], window_refs[window]
    cam = native.camera_from_samples(samples, 800, 800, 64)
    frames = {}
    for mode in ("plain", "skip_empty", "skip_dead", "certify_zero"):
        kw = {} if mode == "plain" else {mode: True}
        frames[mode], st = native.render_image(renderer.coarse, renderer.fine, cam, 128, seed=0, crop=crop, return_stats=True, **kw)
        d = np.abs(frames[mode] - ref)
        print(f"\n{window} {mode}: max|d| {d.max():.2e} mean|d| {d.mean():.2e}, colour heads {st.n_exec_colour} of {st.n_fine_points}")
        assert frames[mode].shape == (crop[3], crop[2], 3)
        assert d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(frames[mode], ref) >= 90.0, (mode, d.max(), d.mean())   # Gate 1
        if mode == "skip_dead":
            if window.startswith("background"):
                assert st.n_exec_colour == 0 and np.all(frames[mode] == 1.0)
            else:
                assert 0 < st.n_exec_colour < st.n_fine_points      # live samples only: every workgroup ends on a partial pass
    for mode in ("skip_empty", "skip_dead", "certify_zero"):
        assert np.array_equal(frames[mode], frames["plain"]), mode
