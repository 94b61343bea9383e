"""Zero-step skipping of the f32 MLP kernels (mlp_f32_core.hip.h tile_steps<*, true>): a k-step whose ReLU'd B register is zero on all
64 lanes is branched round.  fma(a, 0, c) = c, so nothing may change: every test compares a context created with NERF_ZERO_STEP_SKIP=0
(every k-step executed) against a default context in the same process, as uint32 views -- the sign of zero and NaN payloads count -- and
holds the skipping context to the existing bounds against the live oracle.

Engineered networks make the skip do what real weights rarely do: long runs of skipped steps and whole skipped chunks (a), more
consecutive skipped chunks than the LDS ring has slots (b), the four waves of a workgroup skipping different steps between two barriers
(c), a head that sees nothing but zeros (d).  Each asserts from the oracle's outputs that the engineered condition holds."""
import contextlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import SCENE, psnr
from fold_utils import write_random_net

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from zero_skip_cases import DEAD, _copy_net, _edit, _make_case, _sign_points  # noqa: E402

pytestmark = pytest.mark.gpu

VAR = "NERF_ZERO_STEP_SKIP"
N_MAX = 4096
SIZES = (1, 31, 33, 127, 129, N_MAX)


@contextlib.contextmanager
def _env(value, var=VAR):
    """The variable is read at nerf_create: set (or removed) around it only, and restored."""
    old = os.environ.get(var)
    if value is None:
        os.environ.pop(var, None)
    else:
        os.environ[var] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = old


def _renderer(native, skip):
    with _env(None if skip else "0"):
        return native.Renderer(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(on, off, what):
    for name, a, b in zip(("rgb", "sigma"), on, off):
        assert a.shape == b.shape, (what, name)
        differ = _bits(a) != _bits(b)
        assert not differ.any(), f"{what}: {name} differs from the skip-off context in {int(differ.sum())} values"


def _within_bounds(rgb, sg, ergb, esg, what):
    ds, dr = np.abs(sg - esg) / (1 + np.abs(esg)), np.abs(rgb - ergb)
    print(f"\n{what}: sigma rel err max {ds.max():.2e}, rgb err max {dr.max():.2e}")
    assert np.all(np.abs(sg - esg) <= 1e-4 * (1 + np.abs(esg))) and np.all(dr <= 2e-5), what


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(4711)
    return rng.uniform(-2.2, 2.2, size=(3, N_MAX)).astype(np.float32), _dirs(rng, N_MAX)


@pytest.fixture(scope="module")
def scene_pair(native):
    """The lego scene in a skip-off and a default (skip-on) context."""
    off, on = _renderer(native, False), _renderer(native, True)
    off.load_scene(SCENE); on.load_scene(SCENE)
    yield off, on
    off.close(); on.close()


@pytest.fixture(scope="module")
def random_net(tmp_path_factory):
    return write_random_net(tmp_path_factory.mktemp("zskip") / "net", 20240)


@pytest.fixture(scope="module")
def oracle_outputs(oracle, oracle_nets, random_net, points):
    """The oracle on all 4096 points, once per network; every size below is a prefix (each column is computed alone)."""
    return {"coarse": oracle_nets[0].forward_batch(*points), "fine": oracle_nets[1].forward_batch(*points),
            "random": oracle.Net(random_net).forward_batch(*points)}


@pytest.fixture(scope="module")
def random_pair(native, random_net):
    off, on = _renderer(native, False), _renderer(native, True)
    nets = native.load_network_from_dir(off, 0, random_net), native.load_network_from_dir(on, 0, random_net)
    yield nets
    off.close(); on.close()


# ---- 1. forward_batch on real and random networks --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", ("fine", "coarse", "random"))
def test_forward_batch_same_bits_on_and_off(scene_pair, random_pair, points, oracle_outputs, which, n):
    pts, dirs = points
    if which == "random":
        net_off, net_on = random_pair
    else:
        net_off, net_on = (getattr(r, which) for r in scene_pair)
    on = net_on.forward_batch(pts[:, :n], dirs[:n])
    off = net_off.forward_batch(pts[:, :n], dirs[:n])
    _same_bits(on, off, f"{which} n={n}")
    ergb, esg = oracle_outputs[which]
    _within_bounds(on[0], on[1], ergb[:n], esg[:n], f"{which} n={n}")
    if n == N_MAX:  # the sigma-only kernel (nerf_density_batch) reads the same stream
        assert np.array_equal(_bits(net_on.density(pts)), _bits(net_off.density(pts)))


# ---- 2. engineered networks ------------------------------------------------------------------------------------------------------
# the networks and their points live in tests/helpers/zero_skip_cases.py (shared with test_gpu_zero_skip_kernels.py and the CPU proof of the
# engineered conditions, test_zero_skip_cases_cpu.py)


@pytest.fixture(scope="module")
def engineered(oracle, native, random_net, points, tmp_path_factory):
    """Per case: the two loaded contexts' networks, the points and the oracle's outputs on all 4096 of them, computed once."""
    tmp = tmp_path_factory.mktemp("zskip_cases")
    out, keep = {}, []
    for case in "abcd":
        d, twin = _make_case(case, random_net, tmp)
        pts, dirs = points
        live = None
        if case == "c":
            pts, live = _sign_points(np.random.default_rng(99))
        ergb, esg = oracle.Net(d).forward_batch(pts, dirs)
        assert np.isfinite(esg).all() and np.isfinite(ergb).all()
        # the engineered condition, from the oracle's outputs
        if case == "d":
            assert np.all(esg == np.float32(0.7))                      # sigma = relu(alpha bias): nothing of the point reaches the head
            assert ergb.std() > 1e-3                                   # the colour still follows the direction
        else:
            trgb, tsg = oracle.Net(twin).forward_batch(pts, dirs)
            same = np.all(_bits(trgb) == _bits(ergb), axis=1) & (_bits(tsg) == _bits(esg))
            if case == "c":                                            # dense1's kernel is irrelevant exactly where x < 0
                assert np.all(same[~live]) and same[live].mean() < 0.01
            else:                                                      # the consumer's rows of the dead units are irrelevant everywhere
                assert np.all(same)
        assert ergb.std() > 1e-3 and (case == "d" or esg.std() > 0)    # ... and the network still computes something
        off, on = _renderer(native, False), _renderer(native, True)
        keep += [off, on]
        out[case] = (native.load_network_from_dir(off, 0, d), native.load_network_from_dir(on, 0, d), pts, dirs, ergb, esg)
    yield out
    for r in keep:
        r.close()


@pytest.mark.parametrize("case,n", [("a", N_MAX), ("b", N_MAX), ("c", N_MAX), ("c", 128), ("c", 129), ("d", N_MAX)])
def test_engineered_networks_same_bits_on_and_off(engineered, case, n):
    net_off, net_on, pts, dirs, ergb, esg = engineered[case]
    on = net_on.forward_batch(pts[:, :n], dirs[:n])
    off = net_off.forward_batch(pts[:, :n], dirs[:n])
    _same_bits(on, off, f"case {case} n={n}")
    _within_bounds(on[0], on[1], ergb[:n], esg[:n], f"case {case} n={n}")


# ---- 3. a non-finite weight switches the skip off for that network ----------------------------------------------------------------
_COUNTS = re.compile(r"relu_ksteps_executed=(\d+) relu_ksteps_total=(\d+)")
# ReLU k-steps of one wave (32 points) in the full kernel: 128 each for dense1..4, the hidden rows of dense5, dense6, dense7 and viewdirs'
KSTEPS_PER_WAVE = 8 * 128


def _counted_forward(native, capfd, d, pts, dirs):
    """forward_batch in a default (skipping) context that counts its ReLU k-steps (NERF_DEBUG_ZSKIP=1 at nerf_create, one line on stderr
    per launch) -> (rgb, sigma), executed, total: what the context that ran the network decided, not only what the loader's predicate says."""
    with _env(None), _env("1", "NERF_DEBUG_ZSKIP"):
        r = native.Renderer(0)
    with r:
        net = native.load_network_from_dir(r, 0, d)
        capfd.readouterr()
        out = net.forward_batch(pts, dirs)
        counts = _COUNTS.findall(capfd.readouterr().err)
    assert counts, "no k-step counters on stderr"
    return out, sum(int(e) for e, _ in counts), sum(int(t) for _, t in counts)


@pytest.fixture(scope="module")
def dead_register_net(random_net, tmp_path_factory):
    """Units 3 and 7 of dense2 share one B register (mlp_layout.h regFeature: register 3 of tile 0, lane halves 0 and 1); both dead at every
    point, so k-step 3 of dense3 is dead in every wave.  The control: with finite weights a counting default context skips it."""
    d = _copy_net(random_net, str(tmp_path_factory.mktemp("zskip_dead_register") / "finite"))
    _edit(d, "dense2_bias", lambda b: b.__setitem__([3, 7], DEAD))
    return d


VALUES = {"+inf": np.float32(np.inf), "-inf": np.float32(-np.inf), "+nan": np.array([0x7FC00000], np.uint32).view(np.float32)[0]}


@pytest.mark.parametrize("value", list(VALUES))
def test_inf_weight_runs_dense(native, dead_register_net, points, tmp_path, capfd, value):
    """Row 7 of dense3 (the dead register's lane half 1) holds one non-finite weight towards unit 0.  The dense path computes
    fma(w, 0, c) = NaN into unit 0 of dense3 at every point.  Skipping that k-step instead leaves exactly what the finite control
    computes: the control's weight there is multiplied by the same zeros and every other parameter is the same.  So the test is
    sensitive iff the skip-off context's output differs from the control's, which it asserts.  (A NaN need not survive to
    sigma for that -- the integer-max ReLU maps one whose sign bit is set to +0 -- and on MI355X none does: sigma differs from the
    control at 478 of 4096 points for +-inf and at 4050 for +NaN, and is NaN at none.)
    The loader must find the value and the context must run this network with every k-step executed: executed == total in a
    counting default context, where the finite control skips at least that k-step in every wave, and the same bits as the skip-off
    context.  Without the guard the skipping context would return the control's bits, and both assertions would fail."""
    import ctypes as C
    pts, dirs = points
    n_waves = N_MAX // 32
    ctl, c_exec, c_total = _counted_forward(native, capfd, dead_register_net, pts, dirs)
    d = _copy_net(dead_register_net, str(tmp_path / "nonfinite"))
    def kern(w):
        w.reshape(256, 256)[7, 0] = VALUES[value]
    _edit(d, "dense3_kernel", kern)
    eligible = C.c_int(-1)
    assert native.load_library().nerf_debug_zero_skip_network_dir(d.encode(), C.byref(eligible)) == 0 and eligible.value == 0
    a, executed, total = _counted_forward(native, capfd, d, pts, dirs)
    with _renderer(native, False) as off:
        b = native.load_network_from_dir(off, 0, d).forward_batch(pts, dirs)
    print(f"\nfinite control: executed {c_exec} of {c_total} ReLU k-steps; {value}: executed {executed} of {total},"
          f" skip-off NaN in sigma at {int(np.isnan(b[1]).sum())} and in rgb at {int(np.isnan(b[0]).any(axis=1).sum())} of {N_MAX} points, sigma differs from the control at"
          f" {int((_bits(b[1]) != _bits(ctl[1])).sum())}")
    assert c_total == n_waves * KSTEPS_PER_WAVE and c_exec <= c_total - n_waves     # the engineered k-step IS skipped when it may be
    assert np.isfinite(ctl[1]).all()
    assert (_bits(b[1]) != _bits(ctl[1])).any()                                        # executing the k-step shows in the dense output
    assert total == n_waves * KSTEPS_PER_WAVE and executed == total                    # the skipping context ran this network dense
    _same_bits(a, b, value)


# ---- 4. the render modes and the density grid -------------------------------------------------------------------------------------
WINDOWS = {"background 21x13": (3, 5, 21, 13), "edge 48x40": (280, 300, 48, 40)}     # test_gpu_fold.py's two windows


@pytest.fixture(scope="module")
def window_refs(oracle, oracle_nets, samples):
    cam = oracle.camera_from_samples(samples, 800, 800)
    return {k: oracle.render_image(oracle_nets[0], oracle_nets[1], cam, oracle.make_opts(64, 128, crop=c, seed=0)) for k, c in WINDOWS.items()}


@pytest.mark.parametrize("window", list(WINDOWS))
def test_render_modes_equal_the_skip_off_plain_frame(scene_pair, native, samples, window_refs, window):
    off, on = scene_pair
    crop, ref = WINDOWS[window], window_refs[window]
    cam = native.camera_from_samples(samples, 800, 800, 64)
    plain_off = native.render_image(off.coarse, off.fine, cam, 128, seed=0, crop=crop)
    for mode in ("plain", "skip_empty", "skip_dead", "certify_zero"):
        kw = {} if mode == "plain" else {mode: True}
        frame = native.render_image(on.coarse, on.fine, cam, 128, seed=0, crop=crop, **kw)
        d = np.abs(frame - ref)
        print(f"\n{window} {mode}: max|d| {d.max():.2e} mean|d| {d.mean():.2e}")
        assert frame.shape == (crop[3], crop[2], 3)
        assert np.array_equal(_bits(frame), _bits(plain_off)), mode
        assert d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(frame, ref) >= 90.0, (mode, d.max(), d.mean())   # Gate 1


def test_density_grid_same_bits_on_and_off(scene_pair):
    off, on = scene_pair
    lo, step, dims = (-1.1, -0.9, -0.6), (0.27, 0.29, 0.31), (9, 7, 5)
    for which in ("coarse", "fine"):
        s_on, b_on, n_on, _ = getattr(on, which).density_grid(lo, step, dims, threshold=0.5)
        s_off, b_off, n_off, _ = getattr(off, which).density_grid(lo, step, dims, threshold=0.5)
        assert s_on.shape == (5, 7, 9) and np.array_equal(_bits(s_on), _bits(s_off)) and np.array_equal(b_on, b_off) and n_on == n_off
    assert (s_on > 0).any()                                             # the lattice crosses the model
