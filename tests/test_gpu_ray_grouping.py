"""Ray grouping of the f32 ray-mode MLP kernels on the device: a default context (the four waves of a workgroup take one 32-sample segment of
four neighbouring rays, mlp_layout.h) against a NERF_RAY_GROUPING=0 context (128 consecutive samples per workgroup) in the same process.
Every point is evaluated alone, so frames and maps must agree bit for bit (compared as uint32), and the ReLU k-steps a launch executes
(NERF_DEBUG_ZSKIP=1) must be the same numbers: the mapping permutes wave tiles, a difference means one was lost or doubled.

That grouping is really on shows where the tile's composition is visible: skip_empty skips the colour head of workgroup tiles whose 128
sigmas are all zero, and with the "half-space empty" network the number of such tiles is predicted on the CPU for both mappings
(test_ray_grouping_host.py proves the two predictions certain and different) and asserted for both contexts."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import write_random_net

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "tools"))
import ray_grouping_cases as G  # noqa: E402
import zero_skip_cases as Z  # noqa: E402
from scene_utils import random_scene  # noqa: E402
from test_gpu_zero_skip import _bits, _env  # noqa: E402  (its helpers, not its tests)

pytestmark = pytest.mark.gpu

VAR = "NERF_RAY_GROUPING"
_LINE = re.compile(r"nerf zskip: (\S+) relu_ksteps_executed=(\d+) relu_ksteps_total=(\d+)")
SIGMA_RAYS, FULL_RAYS = "nerf_mlp_kernel<sigma,rays>", "nerf_mlp_kernel<full,rays>"
# 384 rays = 96 blocks of four; 273 = 4 x 68 + 1; 5 = one block and one ray.  On lego the first two lie across the model's edge.
WINDOWS = {"24x16": (300, 310, 24, 16), "21x13": (301, 311, 21, 13), "5x1": (330, 340, 5, 1)}
# (coarse, fine, coarse_only): samples per ray 64 / 192 (S = 2 / 6), 64 / 128 (S = 2 / 4), 32 (S = 1), 20 / 70 (no multiple of 32: grouping off)
COUNTS = {"64+128": (64, 128, False), "64+64": (64, 64, False), "32+0": (32, 0, True), "20+50": (20, 50, False)}


class _Ctx:
    """A counting context (NERF_DEBUG_ZSKIP=1) with grouping on (the default) or off.  run() -> (fn's result, [(kernel, executed, total)])."""

    def __init__(self, native, grouping, extra=()):
        env = [(VAR, None if grouping else "0"), ("NERF_DEBUG_ZSKIP", "1"), *extra]
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


def _load(native, ctx, scene):
    if isinstance(scene, str) and os.path.isdir(os.path.join(scene, "coarse")):
        ctx.r.load_scene(scene)
    else:                                                            # one network directory as coarse and fine
        ctx.r.coarse = native.load_network_from_dir(ctx.r, 0, scene)
        ctx.r.fine = native.load_network_from_dir(ctx.r, 1, scene)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    return {"lego": SCENE, "random": str(random_scene(tmp_path_factory.mktemp("raygroup") / "rnd", 321))}


@pytest.fixture(scope="module")
def pairs(native, scenes):
    """scene -> (grouping-off, default) counting contexts"""
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


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    differ = _bits(a) != _bits(b)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values differ, first at {tuple(np.argwhere(differ)[0])}"


def _render(native, samples, r, crop, counts, **kw):
    nc, nf, coarse_only = COUNTS[counts]
    cam = native.camera_from_samples(samples, 800, 800, nc)
    return native.render_image(r.coarse, r.fine, cam, nf, seed=0, crop=crop, coarse_only=coarse_only, **kw)


def _same_render(native, samples, capfd, off, on, crop, counts, what, **kw):
    """One render in both contexts: every returned array bit for bit, and the launches' k-step counters -> (arrays, launches)."""
    a, g_off = off.run(capfd, lambda r: _render(native, samples, r, crop, counts, **kw))
    b, g_on = on.run(capfd, lambda r: _render(native, samples, r, crop, counts, **kw))
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):                                 # (the stats, where asked for, are no array)
            _eq(y, x, f"{what}, output {k}, default / grouping-off")
    assert g_on and len(g_on) == len(g_off), (what, g_on, g_off)
    kernels = {n for n, _, _ in g_on}
    assert kernels <= {SIGMA_RAYS, FULL_RAYS} and (FULL_RAYS in kernels), (what, kernels)     # the ray-mode kernels ran, nothing else
    if not kw.get("skip_empty"):          # a skipped colour head never reaches its k-steps, and WHICH tiles are skipped follows the mapping
        assert g_on == g_off, f"{what}: k-step counters differ: {g_on} / {g_off}"
    else:
        assert [g for g in g_on if g[0] == SIGMA_RAYS] == [g for g in g_off if g[0] == SIGMA_RAYS], what
    return b, g_on


@pytest.mark.parametrize("counts", list(COUNTS))
@pytest.mark.parametrize("scene", ("lego", "random"))
def test_frames_and_maps_same_bits(pairs, native, samples, capfd, scene, counts):
    off, on = pairs(scene)
    for window, crop in WINDOWS.items():
        what = f"{scene} {counts} {window}"
        (plain,), _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " plain")
        assert plain.shape == (crop[3], crop[2], 3) and np.isfinite(plain).all()
        aux, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " plain + maps", aux=True)
        _eq(aux[0], plain, what + " with maps / without")
        (empty,), _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " skip_empty", skip_empty=True)
        _eq(empty, plain, what + " skip_empty / plain")
        eaux, _ = _same_render(native, samples, capfd, off, on, crop, counts, what + " skip_empty + maps", skip_empty=True, aux=True)
        for k in range(3):
            _eq(eaux[k], aux[k], what + f" skip_empty + maps / plain + maps, output {k}")


@pytest.mark.parametrize("scene", ("lego", "random"))
def test_ssaa_same_bits(pairs, native, samples, capfd, scene):
    off, on = pairs(scene)
    crop = WINDOWS["21x13"]                                          # 42 x 26 = 1092 rays
    (frame,), _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{scene} ssaa 2", ssaa=2)
    (empty,), _ = _same_render(native, samples, capfd, off, on, crop, "64+128", f"{scene} ssaa 2 skip_empty", ssaa=2, skip_empty=True)
    assert frame.shape == (13, 21, 3)
    _eq(empty, frame, f"{scene} ssaa 2 skip_empty / plain")


def test_passes_that_end_inside_the_window(pairs, native, samples, capfd):
    """NERF_MAX_RAYS_PER_PASS = 50 (read when a context is created): the 21 x 13 window in six passes of two rows (42 rays = 4 x 10 + 2) and
    one of one row (21 = 4 x 5 + 1) -- every pass has its own grouped part and its own ungrouped tail."""
    off, on = pairs("lego", extra=(("NERF_MAX_RAYS_PER_PASS", "50"),))
    whole_off, whole_on = pairs("lego")
    crop = WINDOWS["21x13"]
    (frame, st), g = _same_render(native, samples, capfd, off, on, crop, "64+128", "passes of 42 rays", return_stats=True)
    assert st.n_passes == 7 and len(g) == 14
    (whole,), _ = _same_render(native, samples, capfd, whole_off, whole_on, crop, "64+128", "one pass")
    _eq(frame, whole, "seven passes / one pass")
    (empty, st), _ = _same_render(native, samples, capfd, off, on, crop, "64+128", "passes of 42 rays, skip_empty", return_stats=True, skip_empty=True)
    assert st.n_passes == 7
    _eq(empty, whole, "seven passes, skip_empty / one pass, plain")


@pytest.mark.parametrize("scene", ("lego", "random"))
def test_shared_origin_ray_batch_same_bits(pairs, native, samples, capfd, scene):
    """130 caller-supplied rays from one origin (the image path's ray-mode launches): 32 blocks of four and two rays."""
    off, on = pairs(scene)
    rng = np.random.default_rng(130)
    origin = np.float32(samples["camera_origin"])
    dirs = (rng.uniform(-1.0, 1.0, size=(130, 3)) - origin).astype(np.float32)
    call = lambda r: native.render_rays(r.coarse, r.fine, origin, dirs, float(samples["near"]), float(samples["far"]), 128, seed=0, aux=True)
    a, g_off = off.run(capfd, call)
    b, g_on = on.run(capfd, call)
    for name, x, y in zip(("rgb", "depth", "opacity"), a, b):
        _eq(y, x, f"{scene} render_rays {name}, default / grouping-off")
    assert np.isfinite(b[0]).all() and b[0].std() > 0
    assert [n for n, _, _ in g_on] == [SIGMA_RAYS, FULL_RAYS] and g_on == g_off, (g_on, g_off)
    assert g_on[0][2] == Z.n_waves(130 * 64) * 7 * 128 and g_on[1][2] == Z.n_waves(130 * 192) * 8 * 128


def test_grouping_is_on_on_the_device(native, oracle, samples, capfd, tmp_path):
    """The half-space-empty network, one row of 16 rays, half of which cross from an empty first segment into density while the others see nothing: the
    workgroup tiles that skip_empty skips are other tiles, and another number of them, under the two mappings.  Both numbers are predicted
    from the oracle's fine samples and the mapping tables (nerf_debug_ray_grouping), and each context must report its own."""
    d = Z._make_case("f", write_random_net(tmp_path / "net", 20240), tmp_path, oracle)[0]
    x0, y0, w, h = G.F_ROW_WINDOW
    n_rays, spr = w * h, 192
    zero, positive = G.case_f_fine_samples(oracle, samples, d, tmp_path / "f_lifted")
    want = {}
    for grouping in (False, True):
        lo, hi = G.empty_tiles(G.table(native, n_rays, spr, grouping), zero, positive)
        assert lo == hi, (grouping, lo, hi)
        want[grouping] = lo
    assert 0 < want[False] < want[True] < G.n_tiles(n_rays, spr), want
    frames = {}
    for grouping in (False, True):
        ctx = _Ctx(native, grouping)
        try:
            _load(native, ctx, d)
            (plain,), _ = ctx.run(capfd, lambda r: (_render(native, samples, r, G.F_ROW_WINDOW, "64+128"),))
            (frame, st), g = ctx.run(capfd, lambda r: _render(native, samples, r, G.F_ROW_WINDOW, "64+128", skip_empty=True, return_stats=True))
        finally:
            ctx.r.close()
        with capfd.disabled():
            print(f"\ncase f {G.F_ROW_WINDOW} grouping {'on' if grouping else 'off'}: n_fine_points {st.n_fine_points} n_colour_skipped_points"
                  f" {st.n_colour_skipped_points}, predicted {128 * want[grouping]}")
        assert st.n_fine_points == n_rays * spr
        assert st.n_colour_skipped_points == 128 * want[grouping], (grouping, st.n_colour_skipped_points, want)
        _eq(frame, plain, f"case f skip_empty / plain, grouping {grouping}")
        frames[grouping] = frame
    _eq(frames[True], frames[False], "case f, default / grouping-off")
    assert (frames[True] != 1.0).any()
