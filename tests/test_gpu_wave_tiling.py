"""Wave tiling of the f32 ray-mode MLP kernels on the device: a default context (in an image pass a wave holds a few samples of each ray of a
block of neighbouring pixels, mlp_layout.h) against a NERF_WAVE_TILING=0 context (32 consecutive samples of one ray) in the same process.
Every point is evaluated alone, so frames and maps must agree bit for bit (compared as uint32) and a launch must count the same TOTAL of ReLU
k-steps (NERF_DEBUG_ZSKIP=1); the EXECUTED k-steps are what tiling is for: fewer on the sampling launch, and inside the float64 bracket formed
over the very waves nerf_debug_wave_tiling reports.

That tiling is really on also shows in skip_empty, which votes over a workgroup tile's 128 points: with the "half-space empty" network the
number of empty tiles is predicted on the CPU for both mappings (test_wave_tiling_host.py proves the two predictions certain and different)
and asserted for both contexts.

Control: with NERF_WAVE_TILING_TEST_CONTROL=1 in the environment the "default" contexts are created with NERF_WAVE_TILING=0 as well; then
test_sampling_launch_executes_fewer_ksteps and test_tiling_is_on_on_the_device must fail (profiles/wavetile_counts.txt records such a run)."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import write_random_net

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "tools"))
import ray_grouping_cases as G  # noqa: E402
import wave_tiling_cases as W  # noqa: E402
import zero_skip_cases as Z  # noqa: E402
from scene_utils import random_scene  # noqa: E402
from test_gpu_ray_grouping import COUNTS, FULL_RAYS, SIGMA_RAYS, _LINE, _eq, _load, _render  # noqa: E402  (its helpers, not its tests)
from test_gpu_zero_skip import _env  # noqa: E402

pytestmark = pytest.mark.gpu

VAR = "NERF_WAVE_TILING"
CONTROL = os.environ.get("NERF_WAVE_TILING_TEST_CONTROL") == "1"
# all at (300, 310) of the 800 x 800 view: on lego the larger ones lie across the model's edge.  32x8 and 8x4: whole 8 x 4 and 4 x 2 blocks;
# 24x16: both kinds tiled; 21x13: the sampling launch in 1 x 4 x 8 with a tail row, the full launch untiled; 12x6: 4 x 4 x 2 with two tail rows;
# 5x1: nothing tiled
WINDOWS = {"32x8": (300, 310, 32, 8), "24x16": (300, 310, 24, 16), "21x13": (300, 310, 21, 13), "12x6": (300, 310, 12, 6),
           "8x4": (300, 310, 8, 4), "5x1": (300, 310, 5, 1)}


class _Ctx:
    """A counting context (NERF_DEBUG_ZSKIP=1) with tiling on (the default) or off.  run() -> (fn's result, [(kernel, executed, total)])."""

    def __init__(self, native, tiling, extra=()):
        self.tiling = tiling and not CONTROL
        env = [(VAR, None if self.tiling else "0"), ("NERF_DEBUG_ZSKIP", "1"), *extra]
        stack = [_env(v, k) for k, v in env]
        for s in stack:
            s.__enter__()
        try:
            self.r = native.Renderer(0)
        finally:
            for s in reversed(stack):
                s.__exit__(None, None, None)

    def run(self, capfd, fn):
        capfd.readouterr()
        out = fn(self.r)
        return out, [(name, int(e), int(t)) for name, e, t in _LINE.findall(capfd.readouterr().err)]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    return {"lego": SCENE, "random": str(random_scene(tmp_path_factory.mktemp("wavetile") / "rnd", 321))}


@pytest.fixture(scope="module")
def pairs(native, scenes):
    """scene -> (tiling-off, default) counting contexts"""
    made = {}

    def get(key, extra=()):
        k = (key, tuple(extra))
        if k not in made:
            off, on = _Ctx(native, False, extra), _Ctx(native, True, extra)
            for c in (off, on):
                _load(native, c, scenes.get(key, key))
            made[k] = (off, on)
        return made[k]

    yield get
    for off, on in made.values():
        off.r.close(); on.r.close()


def _same_render(native, samples, capfd, off, on, crop, counts, what, **kw):
    """One render in both contexts: every returned array bit for bit, and per launch the same kernel and the same total of ReLU k-steps --
    except the full launch's total under skip_empty: a skipped colour head never reaches (or counts) its k-steps, and which workgroup tiles
    are skipped follows the mapping; the sampling launch's total is compared there too -> (arrays, default's launches, tiling-off's launches)."""
    a, g_off = off.run(capfd, lambda r: _render(native, samples, r, crop, counts, **kw))
    b, g_on = on.run(capfd, lambda r: _render(native, samples, r, crop, counts, **kw))
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):                                 # (the stats, where asked for, are no array)
            _eq(y, x, f"{what}, output {k}, default / tiling-off")
    assert g_on and len(g_on) == len(g_off), (what, g_on, g_off)
    kernels = {n for n, _, _ in g_on}
    assert kernels <= {SIGMA_RAYS, FULL_RAYS} and (FULL_RAYS in kernels), (what, kernels)     # the ray-mode kernels ran, nothing else
    totals = lambda g: [(n, t) for n, _, t in g if not (kw.get("skip_empty") and n == FULL_RAYS)]   # a skipped colour head never reaches its
    assert totals(g_on) == totals(g_off), f"{what}: k-step totals differ: {g_on} / {g_off}"          # k-steps, and WHICH tiles are skipped follows the mapping
    return b, g_on, g_off


@pytest.mark.parametrize("counts", list(COUNTS))
@pytest.mark.parametrize("scene", ("lego", "random"))
def test_frames_and_maps_same_bits(pairs, native, samples, capfd, scene, counts):
    off, on = pairs(scene)
    for window, crop in WINDOWS.items():
        what = f"{scene} {counts} {window}"
        (plain,), _, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " plain")
        assert plain.shape == (crop[3], crop[2], 3) and np.isfinite(plain).all()
        aux, _, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " plain + maps", aux=True)
        _eq(aux[0], plain, what + " with maps / without")
        (empty,), _, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " skip_empty", skip_empty=True)
        _eq(empty, plain, what + " skip_empty / plain")
        eaux, _, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " skip_empty + maps", skip_empty=True, aux=True)
        for k in range(3):
            _eq(eaux[k], aux[k], what + f" skip_empty + maps / plain + maps, output {k}")


@pytest.mark.parametrize("scene", ("lego", "random"))
def test_ssaa_same_bits(pairs, native, samples, capfd, scene):
    off, on = pairs(scene)
    for window in ("21x13", "12x6"):                                  # 42 x 26 and 24 x 12 rays
        crop = WINDOWS[window]
        (frame,), _, _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{scene} {window} ssaa 2", ssaa=2)
        (empty,), _, _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{scene} {window} ssaa 2 skip_empty", ssaa=2, skip_empty=True)
        assert frame.shape == (crop[3], crop[2], 3)
        _eq(empty, frame, f"{scene} {window} ssaa 2 skip_empty / plain")


@pytest.mark.parametrize("window,rows", (("24x16", (5, 5, 5, 1)), ("21x13", (6, 6, 1))))
def test_passes_with_tail_rows_and_short_passes(pairs, native, samples, capfd, window, rows):
    """NERF_MAX_RAYS_PER_PASS = 130 (read when a context is created): the 24 x 16 window in three passes of five rows and one of one row, the
    21 x 13 window in two of six rows and one of one -- passes whose last rows % th rows are an untiled tail behind the tiled region, and
    passes shorter than a block is high, which are not tiled at all."""
    off, on = pairs("lego", extra=(("NERF_MAX_RAYS_PER_PASS", "130"),))
    whole_off, whole_on = pairs("lego")
    crop = WINDOWS[window]
    (frame, st), g, _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{window} in passes", return_stats=True)
    assert st.n_passes == len(rows) and len(g) == 2 * len(rows)
    assert [t for _, _, t in g] == [Z.n_waves(r * crop[2] * spr) * layers * 128 for r in rows for spr, layers in ((64, 7), (192, 8))]
    (whole,), _, _ = _same_render(native, samples, capfd, whole_off, whole_on, crop, "64+128", f"{window} in one pass")
    _eq(frame, whole, f"{window}: passes / one pass")
    (empty, st), _, _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{window} in passes, skip_empty", return_stats=True, skip_empty=True)
    assert st.n_passes == len(rows)
    _eq(empty, whole, f"{window}: passes, skip_empty / one pass, plain")


@pytest.mark.parametrize("scene", ("lego", "random"))
def test_ray_batch_is_untiled(pairs, native, samples, capfd, scene):
    """130 caller-supplied rays from one origin: no row width is known, both contexts compose the same waves -- equal executed counters."""
    off, on = pairs(scene)
    rng = np.random.default_rng(130)
    origin = np.float32(samples["camera_origin"])
    dirs = (rng.uniform(-1.0, 1.0, size=(130, 3)) - origin).astype(np.float32)
    call = lambda r: native.render_rays(r.coarse, r.fine, origin, dirs, float(samples["near"]), float(samples["far"]), 128, seed=0, aux=True)
    a, g_off = off.run(capfd, call)
    b, g_on = on.run(capfd, call)
    for name, x, y in zip(("rgb", "depth", "opacity"), a, b):
        _eq(y, x, f"{scene} render_rays {name}, default / tiling-off")
    assert [n for n, _, _ in g_on] == [SIGMA_RAYS, FULL_RAYS] and g_on == g_off, (g_on, g_off)


def test_sampling_launch_executes_fewer_ksteps(pairs, native, samples, capfd):
    """lego, 32 x 8 pixels, 64 + 128 samples: the sampling launch of the default context (8 x 4 pixels x 1 sample per wave) executes strictly fewer
    ReLU k-steps than that of the tiling-off context, and either count lies inside the float64 bracket of zero_skip_cases.py formed over the
    waves that nerf_debug_wave_tiling reports for it (the coarse points from the stage calls: origin + direction x t, rounded separately)."""
    off, on = pairs("lego")
    x0, y0, w, h = crop = WINDOWS["32x8"]
    _, g_on, g_off = _same_render(native, samples, capfd, off, on, crop, "64+128", "lego 32x8")
    cam = native.camera_from_samples(samples, 800, 800, 64)
    d = on.r.stage_ray_dirs(cam, x0, y0, w, h).reshape(-1, 1, 3)
    t = on.r.stage_stratified(cam, x0, y0, w, h, 64, seed=0).reshape(-1, 64, 1)
    pts = (np.float32(samples["camera_origin"]) + (d * t).astype(np.float32)).astype(np.float32).reshape(-1, 3)      # slot order
    pre = Z.preacts_fp64(os.path.join(SCENE, "coarse"), np.ascontiguousarray(pts.T))[:7]
    executed = {}
    for ctx, g in ((off, g_off), (on, g_on)):
        (name, e, total), = [x for x in g if x[0] == SIGMA_RAYS]
        live, dead, tot = W.kstep_bracket(W.table(native, h, w, 64, False, True, ctx.tiling), pre, Z.EPS)
        with capfd.disabled():
            print(f"\nwavetile-count lego 32x8 sampling launch, tiling {'on' if ctx.tiling else 'off'}: executed {e} of {total}; bracket [{live}, {tot - dead}]")
        assert total == tot and live <= e <= tot - dead, (ctx.tiling, live, e, tot - dead)
        executed[ctx is on] = e
    assert executed[True] < executed[False], executed


def test_tiling_is_on_on_the_device(native, oracle, samples, capfd, tmp_path):
    """The half-space-empty network on 16 x 2 pixels: the workgroup tiles that skip_empty skips are other tiles, and another number of them,
    tiled and untiled.  Both numbers are predicted from the oracle's fine samples and the mapping tables (nerf_debug_wave_tiling), and each
    context must report its own."""
    d = Z._make_case("f", write_random_net(tmp_path / "net", 20240), tmp_path, oracle)[0]
    x0, y0, w, h = W.F_BLOCK_WINDOW
    zero, positive = G.case_f_fine_samples(oracle, samples, d, tmp_path / "f_lifted", window=W.F_BLOCK_WINDOW)
    want = {}
    for tiling in (False, True):
        lo, hi = W.empty_tiles(W.table(native, h, w, 192, True, True, tiling), zero, positive)
        assert lo == hi, (tiling, lo, hi)
        want[tiling] = lo
    assert 0 < want[True] < want[False] < W.n_tiles(h, w, 192), want
    frames = {}
    for tiling in (False, True):
        ctx = _Ctx(native, tiling)
        try:
            _load(native, ctx, d)
            (plain,), _ = ctx.run(capfd, lambda r: (_render(native, samples, r, W.F_BLOCK_WINDOW, "64+128"),))
            (frame, st), g = ctx.run(capfd, lambda r: _render(native, samples, r, W.F_BLOCK_WINDOW, "64+128", skip_empty=True, return_stats=True))
        finally:
            ctx.r.close()
        with capfd.disabled():
            print(f"\ncase f {W.F_BLOCK_WINDOW} tiling {'on' if tiling else 'off'}: n_fine_points {st.n_fine_points} n_colour_skipped_points"
                  f" {st.n_colour_skipped_points}, predicted {128 * want[tiling]}")
        assert st.n_fine_points == w * h * 192
        assert st.n_colour_skipped_points == 128 * want[tiling], (tiling, st.n_colour_skipped_points, want)
        _eq(frame, plain, f"case f skip_empty / plain, tiling {tiling}")
        frames[tiling] = frame
    _eq(frames[True], frames[False], "case f, default / tiling-off")
    assert (frames[True] != 1.0).any()
