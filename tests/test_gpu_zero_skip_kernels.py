"""Zero-step skipping (mlp_f32_core.hip.h tile_steps<*, true>) in EVERY f32 kernel that skips, counted, and at the float edges.

test_gpu_zero_skip.py sends its engineered networks through forward_batch (nerf_mlp_kernel<full,points>) alone.  Here they go through the
other eight instantiations as well -- <sigma,points> (density), <sigma,grid> (density_grid), <sigma,rays> / <full,rays> (renders, with and
without skip_empty's pipe_restart), nerf_trunk_seq_kernel<sigma> / <export> (skip_dead) and <sigma,list> / <full,list>
(certify_zero) -- always as a NERF_ZERO_STEP_SKIP=0 context against a default one in the same process, compared as uint32 views.  Every
context counts (NERF_DEBUG_ZSKIP=1: one stderr line per launch that names the instantiation), and every test asserts from those lines that
the kernels it is about did launch, in both contexts: a test that silently went through another kernel fails.

The counters are predicted, not only read (part C): exactly on the engineered networks, and on ordinary ones inside a float64 bracket that
test_zero_skip_cases_cpu.py proves tight (at most 0.1 % of the k-steps uncertain, at least 1 % certainly dead).  The skip-off context is
the control: executed == total there, which lies outside every one of these bounds.  Bit-identity says "skips nothing live", the counts say
"skips nearly everything dead".

Float edges (forward_batch and density only; the render loops depend on sigma): subnormal and signed-zero biases that survive only if
neither path flushes them (case e), non-finite and huge coordinates at ten points of a batch, finite weights whose activations overflow.
What the MI355X does there is recorded in profiles/zskip_counts.txt.

render_rays turns its samples into points: it reaches the two point kernels with other batch sizes, and is compared on and off as well.
Not here: render_rays with skip_dead -- the library refuses the skip modes for ray batches (test_ray_batch_host.py asserts that)."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import SCENE, psnr
from fold_utils import write_random_net

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import zero_skip_cases as Z  # noqa: E402
from test_gpu_zero_skip import _bits, _env, _renderer, _same_bits, _within_bounds  # noqa: E402  (its helpers, not its tests)

pytestmark = pytest.mark.gpu

N_MAX = Z.N_MAX
_LINE = re.compile(r"nerf zskip: (\S+) relu_ksteps_executed=(\d+) relu_ksteps_total=(\d+)")
K = "nerf_mlp_kernel"
FULL_POINTS, SIGMA_POINTS, SIGMA_GRID = f"{K}<full,points>", f"{K}<sigma,points>", f"{K}<sigma,grid>"
SIGMA_RAYS, FULL_RAYS, SIGMA_LIST, FULL_LIST = f"{K}<sigma,rays>", f"{K}<full,rays>", f"{K}<sigma,list>", f"{K}<full,list>"
SEQ_SIGMA, SEQ_EXPORT = "nerf_trunk_seq_kernel<sigma>", "nerf_trunk_seq_kernel<export>"
ALL_NINE = {FULL_POINTS, SIGMA_POINTS, SIGMA_GRID, SIGMA_RAYS, FULL_RAYS, SIGMA_LIST, FULL_LIST, SEQ_SIGMA, SEQ_EXPORT}
LAUNCHED = {False: {}, True: {}}          # skip off / on -> instantiation -> launches seen by this module, printed when it ends


class _Ctx:
    """One counting context.  run() -> (what fn returned, [(instantiation, executed, total)] of the launches it made)."""

    def __init__(self, native, skip):
        with _env("1", "NERF_DEBUG_ZSKIP"):
            self.r = _renderer(native, skip)
        self.skip = skip

    def run(self, capfd, fn):
        capfd.readouterr()
        out = fn(self.r)
        got = [(name, int(e), int(t)) for name, e, t in _LINE.findall(capfd.readouterr().err)]
        for name, e, t in got:
            assert name in ALL_NINE, name
            assert e <= t and (self.skip or e == t), (name, e, t, "the skip-off context executes every k-step")
            LAUNCHED[self.skip][name] = LAUNCHED[self.skip].get(name, 0) + 1
        return out, got


def _say(capfd, text):
    """Print past capfd (the next run() would swallow it): the figures of profiles/zskip_counts.txt come from these lines."""
    with capfd.disabled():
        print("\n" + text)


def _count(got, name):
    """(executed, total) summed over the launches of one instantiation."""
    return sum(e for n, e, _ in got if n == name), sum(t for n, _, t in got if n == name)


def _launched(got_off, got_on, *names):
    for got, ctx in ((got_off, "skip-off"), (got_on, "default")):
        seen = {n for n, _, _ in got}
        assert set(names) <= seen, f"{ctx} context: {sorted(set(names) - seen)} did not launch (launched: {sorted(seen)})"


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    differ = _bits(a) != _bits(b)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, first at {tuple(np.argwhere(differ)[0])}"


@pytest.fixture(scope="module")
def random_net(tmp_path_factory):
    return write_random_net(tmp_path_factory.mktemp("zskip_k") / "net", 20240)


@pytest.fixture(scope="module")
def pairs(native, oracle, random_net, tmp_path_factory):
    """key -> the (skip-off, default) pair of counting contexts with that network loaded as coarse AND fine: a case letter, "random",
    "overflow", or "lego" (the scene's two networks)."""
    tmp = tmp_path_factory.mktemp("zskip_k_cases")
    made = {}

    def get(key):
        if key not in made:
            if key in Z.CASES:
                d = Z._make_case(key, random_net, tmp, oracle)[0]
            elif key == "overflow":       # finite weights, activations that leave f32: h1 ~ 1e19, h2 ~ 1e38 and beyond
                d = Z._copy_net(random_net, str(tmp / key))
                for name in ("dense1_kernel", "dense2_kernel"):
                    Z._edit(d, name, lambda w: w.__setitem__(slice(None), w * np.float32(1e19)))
            else:
                d = random_net if key == "random" else None
            off, on = _Ctx(native, False), _Ctx(native, True)
            for c in (off, on):
                if d is None:
                    c.r.load_scene(SCENE)
                else:
                    c.r.coarse = native.load_network_from_dir(c.r, 0, d)
                    c.r.fine = native.load_network_from_dir(c.r, 1, d)
            made[key] = types.SimpleNamespace(off=off, on=on, dir=d)
        return made[key]

    yield get
    for p in made.values():
        p.off.r.close(); p.on.r.close()
    for skip in (False, True):
        print(f"\nzskip launches, {'default' if skip else 'skip-off'} contexts: " + ", ".join(f"{k} x{v}" for k, v in sorted(LAUNCHED[skip].items())))


def _lattice_points(lo, step, dims):
    """The lattice of density_grid as the header builds it: per coordinate the f32 product step * float(i), then the f32 sum with lo; x fastest."""
    ax = [np.float32(s) * np.arange(n, dtype=np.float32) + np.float32(l) for l, s, n in zip(lo, step, dims)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)]).astype(np.float32)


LATTICE = ((-1.1, -0.9, -0.6), (0.27, 0.29, 0.31), (9, 7, 5))               # straddles x = 0; 315 cells = 3 workgroup tiles, the last one ragged
# case c's counts: x fastest and 64 wide -- the first wave of every row has x < 0 alone, the second one holds x > 0; 384 cells = 12 whole waves
ROW_LATTICE = ((-1.6, -0.5, 0.2), (0.05, 0.4, 0.7), (64, 3, 2))


# ---- B. engineered networks through every instantiation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", "abcde")
def test_density_same_bits_on_off_and_as_forward_batch(pairs, capfd, case):
    P = pairs(case)
    pts, dirs, _ = Z.case_points(case)
    (_, sg), g_fwd = P.on.run(capfd, lambda r: r.coarse.forward_batch(pts, dirs))
    g_on, g_off = list(g_fwd), []
    for n in (N_MAX, 128, 129):
        s_on, g = P.on.run(capfd, lambda r: r.coarse.density(pts[:, :n])); g_on += g
        s_off, g = P.off.run(capfd, lambda r: r.coarse.density(pts[:, :n])); g_off += g
        _eq(s_on, s_off, f"case {case} density n={n} on / off")
        _eq(s_on, sg[:n], f"case {case} density n={n} / forward_batch's sigma")
    _launched(g_off, g_on, SIGMA_POINTS)
    assert FULL_POINTS in {n for n, _, _ in g_fwd}


@pytest.mark.parametrize("case", "abcde")
def test_density_grid_same_bits_on_off_and_as_density(pairs, capfd, case):
    P = pairs(case)
    lo, step, dims = LATTICE
    (s_on, b_on, n_on, _), g_on = P.on.run(capfd, lambda r: r.coarse.density_grid(lo, step, dims, threshold=0.5))
    (s_off, b_off, n_off, _), g_off = P.off.run(capfd, lambda r: r.coarse.density_grid(lo, step, dims, threshold=0.5))
    assert s_on.shape == (5, 7, 9)
    _eq(s_on, s_off, f"case {case} grid sigma on / off")
    assert np.array_equal(b_on, b_off) and n_on == n_off == int((s_on > 0.5).sum())
    pts = _lattice_points(lo, step, dims)
    assert (pts[0] < 0).any() and (pts[0] > 0).any()
    _eq(s_on.reshape(-1), P.on.r.coarse.density(pts), f"case {case} grid sigma / density at the same points")
    _launched(g_off, g_on, SIGMA_GRID)


MODES = {"plain": (SIGMA_RAYS, FULL_RAYS), "skip_empty": (SIGMA_RAYS, FULL_RAYS), "skip_dead": (SEQ_SIGMA, SEQ_EXPORT),
         "certify_zero": (SIGMA_LIST, FULL_LIST)}


def _render(native, samples, r, crop, mode, stats=False):
    cam = native.camera_from_samples(samples, 800, 800, 64)
    kw = {} if mode == "plain" else {mode: True}
    return native.render_image(r.coarse, r.fine, cam, 128, seed=0, crop=crop, return_stats=stats, **kw)


@pytest.mark.parametrize("window", list(Z.WINDOWS))
@pytest.mark.parametrize("case", "abcde")
def test_render_modes_equal_the_skip_off_plain_frame(pairs, native, oracle, samples, capfd, case, window):
    """The case as coarse and as fine network, 64 + 128 samples, seed 0.  Every mode, in both contexts, returns the bits of the skip-off
    context's plain frame, and that frame meets Gate 1 against the oracle rendering the same networks."""
    P = pairs(case)
    crop = Z.WINDOWS[window]
    plain_off = None
    for mode, kernels in MODES.items():
        f_off, g_off = P.off.run(capfd, lambda r: _render(native, samples, r, crop, mode))
        f_on, g_on = P.on.run(capfd, lambda r: _render(native, samples, r, crop, mode))
        if mode == "plain":
            plain_off = f_off
        assert f_on.shape == (crop[3], crop[2], 3)
        _eq(f_off, plain_off, f"case {case} {window} {mode}, skip-off context / its plain frame")
        _eq(f_on, plain_off, f"case {case} {window} {mode}, default context / the skip-off plain frame")
        _launched(g_off, g_on, *kernels)
    onet = oracle.Net(P.dir)
    ref = oracle.render_image(onet, onet, oracle.camera_from_samples(samples, 800, 800), oracle.make_opts(64, 128, crop=crop, seed=0))
    d = np.abs(plain_off - ref)
    _say(capfd, f"case {case} {window}: plain frame vs oracle max|d| {d.max():.2e} mean|d| {d.mean():.2e} psnr {psnr(plain_off, ref):.1f}; non-white pixels {int((ref != 1).any(axis=2).sum())}")
    assert d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(plain_off, ref) >= 90.0, (d.max(), d.mean())      # Gate 1


@pytest.mark.parametrize("case", "abcde")
def test_render_rays_same_bits_on_and_off(pairs, native, samples, capfd, case):
    """130 caller-supplied rays (a ragged tail behind one 128-ray tile row) with per-ray origins and per-ray (near, far)."""
    P = pairs(case)
    rng = np.random.default_rng(130)
    origins = (np.float32(samples["camera_origin"]) + rng.uniform(-0.3, 0.3, size=(130, 3))).astype(np.float32)
    dirs = (rng.uniform(-1.0, 1.0, size=(130, 3)) - origins).astype(np.float32)
    bounds = np.stack([rng.uniform(1.5, 2.5, 130), rng.uniform(5.0, 6.5, 130)], axis=1).astype(np.float32)
    call = lambda r: native.render_rays(r.coarse, r.fine, origins, dirs, 2.0, 6.0, 128, bounds=bounds, seed=0, aux=True)
    out_off, g_off = P.off.run(capfd, call)
    out_on, g_on = P.on.run(capfd, call)
    for name, a, b in zip(("rgb", "depth", "opacity"), out_on, out_off):
        _eq(a, b, f"case {case} render_rays {name} on / off")
    assert np.isfinite(out_on[0]).all() and out_on[0].std() > 0
    _launched(g_off, g_on, SIGMA_POINTS, FULL_POINTS)          # a ray batch's samples are made into points: the point kernels, 64 and 192 per ray
    assert _count(g_on, SIGMA_POINTS)[1] == Z.n_waves(130 * 64) * 7 * 128 and _count(g_on, FULL_POINTS)[1] == Z.n_waves(130 * 192) * 8 * 128


def test_half_space_empty_skip_modes(pairs, native, samples, capfd):
    """Case f: sigma is exactly 0 on x < 0 and the window's right-hand columns see nothing else.  skip_empty then restarts the weight
    pipeline (pipe_restart) behind tiles whose every wave skipped all of dense1's chunks, skip_dead switches between the trunk and the
    colour stream with rays that have no live sample next to rays that have."""
    P = pairs("f")
    crop = Z.F_WINDOW
    plain_off, g0 = P.off.run(capfd, lambda r: _render(native, samples, r, crop, "plain"))
    plain_on, g1 = P.on.run(capfd, lambda r: _render(native, samples, r, crop, "plain"))
    _eq(plain_on, plain_off, "case f plain on / off")
    _launched(g0, g1, SIGMA_RAYS, FULL_RAYS)
    assert (plain_off[:, -11:] == 1.0).all() and (plain_off != 1.0).any()          # white where nothing but x < 0 is seen, the model elsewhere
    for mode in ("skip_empty", "skip_dead"):
        (f_off, st_off), g_off = P.off.run(capfd, lambda r: _render(native, samples, r, crop, mode, stats=True))
        (f_on, st_on), g_on = P.on.run(capfd, lambda r: _render(native, samples, r, crop, mode, stats=True))
        _eq(f_off, plain_off, f"case f {mode}, skip-off context / plain")
        _eq(f_on, plain_off, f"case f {mode}, default context / the skip-off plain frame")
        _launched(g_off, g_on, *MODES[mode])
        for st in (st_off, st_on):
            _say(capfd, f"case f {mode}: n_fine_points {st.n_fine_points} n_colour_skipped_points {st.n_colour_skipped_points} n_exec_colour {st.n_exec_colour}")
            if mode == "skip_empty":
                assert 0 < st.n_colour_skipped_points < st.n_fine_points            # pipe_restart ran, behind skipped chunks, and not everywhere
            else:
                assert 0 < st.n_exec_colour < st.n_fine_points
        e, t = _count(g_on, MODES[mode][1])
        assert e < t                                                                # ... and the default context did skip k-steps in that kernel


# ---- C.1 engineered counts are exact -------------------------------------------------------------------------------------------------------
def _calls(case):
    """(label, fn(renderer), instantiation, ReLU-input layers, waves, k-steps that are dead by construction) for the three point entry points."""
    pts, dirs, live = Z.case_points(case)
    lo, step, dims = ROW_LATTICE if case == "c" else LATTICE
    n_cells = int(np.prod(dims))
    if case == "c":       # every k-step of dense1 in a wave that sees x <= 0 alone
        dead_pts, dead_grid = Z.dead_wave_steps(live), Z.dead_wave_steps(_lattice_points(lo, step, dims)[0] > 0)
        assert dead_pts == 128 * 64 and dead_grid == 128 * 6
    else:                 # b: all of dense4, e: all of dense7, in every wave (padding waves included: they repeat the last point)
        dead_pts, dead_grid = 128 * Z.n_waves(N_MAX), 128 * Z.n_waves(n_cells)
    return [("forward_batch", lambda r: r.coarse.forward_batch(pts, dirs), FULL_POINTS, 8, Z.n_waves(N_MAX), dead_pts),
            ("density", lambda r: r.coarse.density(pts), SIGMA_POINTS, 7, Z.n_waves(N_MAX), dead_pts),
            ("density_grid", lambda r: r.coarse.density_grid(lo, step, dims), SIGMA_GRID, 7, Z.n_waves(n_cells), dead_grid)]


@pytest.mark.parametrize("case", "bce")
def test_engineered_counts(pairs, capfd, case):
    P = pairs(case)
    for label, fn, kernel, layers, waves, dead in _calls(case):
        total = waves * layers * 128
        _, g_on = P.on.run(capfd, fn)
        _, g_off = P.off.run(capfd, fn)
        (e_on, t_on), (e_off, t_off) = _count(g_on, kernel), _count(g_off, kernel)
        _say(capfd, f"zskip-count case {case} {label} {kernel}: executed {e_on} of {t_on}, dead by construction {dead}; skip-off executed {e_off} of {t_off}")
        assert len(g_on) == len(g_off) == 1
        assert t_on == total and e_on <= total - dead, (label, e_on, t_on, dead)
        assert t_off == total and e_off == total, (label, e_off, t_off)


# ---- C.2 counts on ordinary networks are bracketed --------------------------------------------------------------------------------------------
BATCHES = {"rays": Z.ray_points, "uniform": lambda: Z.uniform_points()}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("net", ("coarse", "fine", "random"))
def test_counts_inside_the_float64_bracket(pairs, random_net, capfd, net, batch):
    """certain_live <= executed <= total - certain_dead, the bracket from float64 pre-activations (eps = 1e-3; its tightness on these six
    pairs is test_zero_skip_cases_cpu.py's).  The skip-off context executes `total`, above the bracket."""
    P = pairs("random" if net == "random" else "lego")
    which = "coarse" if net == "random" else net
    pts, dirs = BATCHES[batch]()
    pre = Z.preacts_fp64(random_net if net == "random" else os.path.join(SCENE, net), pts)
    for label, fn, kernel, layers in (("forward_batch", lambda r: getattr(r, which).forward_batch(pts, dirs), FULL_POINTS, 8),
                                      ("density", lambda r: getattr(r, which).density(pts), SIGMA_POINTS, 7)):
        live, dead, total = Z.kstep_bracket(pre[:layers])
        _, g_on = P.on.run(capfd, fn)
        _, g_off = P.off.run(capfd, fn)
        (e_on, t_on), (e_off, t_off) = _count(g_on, kernel), _count(g_off, kernel)
        _say(capfd, f"zskip-count {net} {batch} {label} {kernel}: executed {e_on} of {t_on}; bracket [{live}, {total - dead}]"
              f" (certainly dead {dead}, uncertain {total - live - dead}); skip-off executed {e_off} of {t_off}")
        assert len(g_on) == len(g_off) == 1
        assert t_on == total and live <= e_on <= total - dead, (label, live, e_on, total - dead)
        assert t_off == total and e_off == total and e_off > total - dead, (label, e_off, t_off)


# ---- C.3 float edges -----------------------------------------------------------------------------------------------------------------------
def test_subnormal_biases_survive_both_paths(pairs, oracle, capfd):
    """Case e: dense7's accumulators hold its biases -- subnormals of both signs, +0, -0 -- through 128 k-steps that the default context
    skips and the skip-off context executes as fma(a, +0, c).  sigma = 2^120 sum max(b7, 0) = 0.0918: a path that flushes subnormals
    (in the MFMA's C input or result, in relu() or in the alpha head) returns 0 instead and misses the oracle by 0.09."""
    P = pairs("e")
    pts, dirs, _ = Z.case_points("e")
    ergb, esg = oracle.Net(P.dir).forward_batch(pts, dirs)
    on, g_on = P.on.run(capfd, lambda r: r.coarse.forward_batch(pts, dirs))
    off, g_off = P.off.run(capfd, lambda r: r.coarse.forward_batch(pts, dirs))
    _say(capfd, f"zskip-edge case e: sigma default {on[1][0]!r} skip-off {off[1][0]!r} oracle {esg[0]!r} float64 {Z.subnormal_sigma_fp64()!r}")
    _same_bits(on, off, "case e")
    _within_bounds(on[0], on[1], ergb, esg, "case e, default context")
    _within_bounds(off[0], off[1], ergb, esg, "case e, skip-off context")
    d_on, g = P.on.run(capfd, lambda r: r.coarse.density(pts)); g_on += g
    d_off, g = P.off.run(capfd, lambda r: r.coarse.density(pts)); g_off += g
    _eq(d_on, on[1], "case e density / forward_batch's sigma"); _eq(d_off, d_on, "case e density on / off")
    _launched(g_off, g_on, FULL_POINTS, SIGMA_POINTS)


@pytest.mark.parametrize("net", ("random", "fine"))
def test_poisoned_points_stay_in_their_columns(pairs, capfd, net):
    """Ten points of the batch carry a NaN (either sign), an infinity, 1e30, 3e38, 2049, the smallest subnormal or -0.0 in one coordinate.
    The loaders' guard reads weights only: the skip is on.  Every other point keeps the bits it has in the clean batch (columns are
    independent), the two contexts agree in every bit at every point -- the poisoned ones too --, density is forward_batch's sigma, and
    the calls return."""
    P = pairs("random" if net == "random" else "lego")
    which = "coarse" if net == "random" else net
    clean, dirs = Z.uniform_points()
    pts, _, hit = Z.poisoned_points()
    fwd = lambda p: (lambda r: getattr(r, which).forward_batch(p, dirs))
    c_on, _ = P.on.run(capfd, fwd(clean)); c_off, _ = P.off.run(capfd, fwd(clean))
    p_on, g_on = P.on.run(capfd, fwd(pts)); p_off, g_off = P.off.run(capfd, fwd(pts))
    d_on, g = P.on.run(capfd, lambda r: getattr(r, which).density(pts)); g_on += g
    d_off, g = P.off.run(capfd, lambda r: getattr(r, which).density(pts)); g_off += g
    for i, v in zip(Z.POISON_AT, Z.POISON):
        _say(capfd, f"zskip-edge {net} point {i} coordinate {v!r}: default sigma {p_on[1][i]!r} rgb {p_on[0][i]}, skip-off sigma {p_off[1][i]!r} rgb {p_off[0][i]}")
    for name, k in (("rgb", 0), ("sigma", 1)):
        _eq(p_on[k][~hit], c_on[k][~hit], f"{net} {name} of the unpoisoned points, default context, poisoned / clean batch")
        _eq(p_off[k][~hit], c_off[k][~hit], f"{net} {name} of the unpoisoned points, skip-off context, poisoned / clean batch")
    _same_bits(p_on, p_off, f"{net} poisoned batch")
    _eq(d_on, p_on[1], f"{net} density / forward_batch's sigma, default context")
    _eq(d_off, p_off[1], f"{net} density / forward_batch's sigma, skip-off context")
    assert (_bits(p_on[1][hit]) != _bits(c_on[1][hit])).any()                      # the poison does reach the outputs of its own points
    _launched(g_off, g_on, FULL_POINTS, SIGMA_POINTS)
    e, t = _count(g_on, FULL_POINTS)
    assert e < t                                                                    # the skip was on


def test_overflowing_activations_same_bits(pairs, native, capfd):
    """dense1 and dense2 scaled by 1e19: every parameter is finite, so the loaders keep the skip on; the activations reach inf and NaN
    all the same.  fma(a, 0, c) = c also for a non-finite c: on and off agree in every bit."""
    P = pairs("overflow")
    eligible = C.c_int(-1)
    assert native.load_library().nerf_debug_zero_skip_network_dir(P.dir.encode(), C.byref(eligible)) == 0 and eligible.value == 1
    pts, dirs = Z.uniform_points()
    on, g_on = P.on.run(capfd, lambda r: r.coarse.forward_batch(pts, dirs))
    off, g_off = P.off.run(capfd, lambda r: r.coarse.forward_batch(pts, dirs))
    d_on, g = P.on.run(capfd, lambda r: r.coarse.density(pts)); g_on += g
    d_off, g = P.off.run(capfd, lambda r: r.coarse.density(pts)); g_off += g
    bad = ~np.isfinite(off[1]) | ~np.isfinite(off[0]).all(axis=1)
    e, t = _count(g_on, FULL_POINTS)
    _say(capfd, f"zskip-edge overflow: skip-off output non-finite at {int(bad.sum())} of {N_MAX} points (sigma NaN {int(np.isnan(off[1]).sum())}, inf {int(np.isinf(off[1]).sum())});"
          f" default context executed {e} of {t}")
    assert bad.any()
    _same_bits(on, off, "overflow")
    _eq(d_on, on[1], "overflow density / forward_batch's sigma"); _eq(d_off, d_on, "overflow density on / off")
    _launched(g_off, g_on, FULL_POINTS, SIGMA_POINTS)
