"""Depth ordering of the fine f32 launch of an image pass (mlp_layout.h DepthOrder): the samples of every 8 x 4 pixel block are merged by
depth on the device (sampling_kernels.hip k_depth_order) and the block's waves are cut from that order, and the persistent workgroups rotate
through the tiles of a round (mlp_layout.h rotated_tile).

  1. the order kernel alone (nerf_stage_depth_order) against np.lexsort over (sample, ray-in-block, t viewed as uint32) per block, exact
     equality, on real lego sample positions and on bits that are no ascending rows: ties, equal t across rays, NaN, -0.0, a swapped pair;
     every table is also checked to be a permutation of its region's slots;
  2. a default context against a NERF_DEPTH_ORDER=0 context in the same process: every point is evaluated alone, so frames, maps, RGBA8 words
     and SSAA frames agree bit for bit (compared as uint32), every launch is the same kernel with the same TOTAL of ReLU k-steps
     (NERF_DEBUG_ZSKIP=1), windows that are not ordered execute the same k-steps too, and skip_empty renders -- whose mapping does not
     change -- skip the same number of colour heads;
  3. it is really on: the fine launch of lego 32 x 8 at 64 + 128 EXECUTES strictly fewer ReLU k-steps by default, and either count lies inside
     the float64 bracket formed over the waves that the returned table (default) or nerf_debug_wave_tiling (switched off) describes;
  4. tile rotation: a default context against a NERF_TILE_ROTATION=0 context, same bits and the same executed and total k-steps per launch.

Control: with NERF_DEPTH_ORDER_TEST_CONTROL=1 in the environment the "default" contexts are created with NERF_DEPTH_ORDER=0 as well; then
test_fine_launch_executes_fewer_ksteps must fail: both contexts then take the static table, execute the same k-steps, and the final '<' does not hold (profiles/depthorder_counts.txt records such a run)."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "tools"))
import wave_tiling_cases as W  # noqa: E402
import zero_skip_cases as Z  # noqa: E402
from render_restatement import GpuBackend, restate  # noqa: E402
from test_gpu_ray_grouping import COUNTS, FULL_RAYS, SIGMA_RAYS, _LINE, _eq, _render  # noqa: E402  (its helpers, not its tests)
from test_gpu_zero_skip import _env  # noqa: E402

pytestmark = pytest.mark.gpu

CONTROL = os.environ.get("NERF_DEPTH_ORDER_TEST_CONTROL") == "1"
# all at (300, 310) of the 800 x 800 view, as the wave-tiling tests: 32x8, 24x16 and 8x4 are ordered (whole 8 x 4 blocks), 21x13 and 12x6 are
# not (the width is no multiple of 8), 5x1 neither (one row)
ORDERED = {"32x8": (300, 310, 32, 8), "24x16": (300, 310, 24, 16), "8x4": (300, 310, 8, 4)}
STATIC = {"21x13": (300, 310, 21, 13), "12x6": (300, 310, 12, 6), "5x1": (300, 310, 5, 1)}


# ---- 1. the order kernel ------------------------------------------------------------------------------------------------------------------
def expected_table(t):
    """t (rows, rw, spr) float32 -> the table of the first (rows // 4) * 4 rows: per 8 x 4 block, row-major, the slots ray * spr + sample in
    ascending (bits of t, ray-in-block row-major, sample) order."""
    rows, rw, spr = t.shape
    bits = np.ascontiguousarray(t, dtype=np.float32).view(np.uint32)
    slot = np.arange(rows * rw * spr, dtype=np.int64).reshape(rows, rw, spr)
    ray = np.repeat(np.arange(32), spr)
    smp = np.tile(np.arange(spr), 32)
    out = []
    for by in range(rows // 4):
        for bx in range(rw // 8):
            b = bits[4 * by:4 * by + 4, 8 * bx:8 * bx + 8].reshape(-1)
            s = slot[4 * by:4 * by + 4, 8 * bx:8 * bx + 8].reshape(-1)
            out.append(s[np.lexsort((smp, ray, b))])
    return np.concatenate(out).astype(np.uint32)


def _check_table(r, t, what):
    t = np.ascontiguousarray(t, dtype=np.float32)
    rows, rw, spr = t.shape
    got = r.stage_depth_order(t)
    n = (rows // 4) * 4 * rw * spr
    assert got.shape == (n,) and got.dtype == np.uint32, what
    for b, block in enumerate(got.reshape(-1, 32 * spr)):               # a permutation of each block's slots
        by, bx = divmod(b, rw // 8)
        want = (((4 * by + np.arange(4))[:, None, None] * rw + (8 * bx + np.arange(8))[None, :, None]) * spr + np.arange(spr)).reshape(-1)
        assert np.array_equal(np.sort(block), np.sort(want).astype(np.uint32)), f"{what}: block {b} is no permutation of its slots"
    assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32)), f"{what}: no permutation of the region's slots"
    want = expected_table(t)
    differ = got != want
    assert not differ.any(), f"{what}: {int(differ.sum())} of {n} entries differ from np.lexsort, first at {int(np.argmax(differ))}"
    return got


@pytest.fixture(scope="module")
def ctx(native):
    with native.Renderer(0) as r:
        r.load_scene(SCENE)
        yield r


@pytest.fixture(scope="module")
def lego_t(native, samples, ctx):
    """(window, nc, nf) -> the fine pass's merged, sorted t of that window from the stage calls, (h, w, nc + nf)"""
    made = {}

    def get(w, h, nc, nf):
        if (w, h, nc, nf) not in made:
            cam = native.camera_from_samples(samples, 800, 800, nc)
            made[(w, h, nc, nf)] = restate(GpuBackend(native, ctx), cam, nc, nf, (300, 310, w, h), 0)
        return made[(w, h, nc, nf)]

    return get


@pytest.mark.parametrize("w,h", ((8, 4), (16, 8)))
@pytest.mark.parametrize("nc,nf", ((64, 128), (16, 16)))
def test_order_kernel_on_lego_samples(ctx, lego_t, w, h, nc, nf):
    t = lego_t(w, h, nc, nf)["t_fine"].reshape(h, w, nc + nf)
    assert (np.diff(t, axis=2) >= 0).all()                               # what the resampler writes: ascending rows
    _check_table(ctx, t, f"lego {w}x{h} {nc}+{nf}")


def _synthetic(rows, rw, spr, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.uniform(2.0, 6.0, size=(rows, rw, spr)).astype(np.float32), axis=2)


def test_order_kernel_all_equal_t(ctx):
    _check_table(ctx, np.full((4, 8, 64), 3.25, np.float32), "all-equal t")        # the order is (ray, sample): the identity per block
    _check_table(ctx, np.full((8, 16, 32), 3.25, np.float32), "all-equal t, four blocks")


def test_order_kernel_equal_t_across_rays(ctx):
    t = _synthetic(4, 8, 64, 1)
    t[:] = t[0, 0]                                                        # every ray holds the same ascending row
    _check_table(ctx, t, "equal t across rays")
    t = _synthetic(8, 8, 64, 2)
    t[1, 3] = t[2, 5]; t[5, 0] = t[2, 5]                                  # three equal rays, two of them in one block
    _check_table(ctx, t, "equal rays within and across blocks")


def test_order_kernel_nan_and_negative_zero(ctx):
    t = _synthetic(4, 16, 64, 3)
    t[2, 9, 17] = np.float32("nan")                                        # bits 0x7FC00000: behind every finite positive t
    t[1, 12, 0] = np.float32(-0.0)                                         # bits 0x80000000: behind every positive pattern, that NaN included
    got = _check_table(ctx, t, "one NaN and one -0.0")
    spr = 64
    block1 = got[32 * spr:]                                                # both lie in block 1 (columns 8..15)
    assert t[2, 9, 17:18].view(np.uint32)[0] == 0x7FC00000 and block1[-2] == (2 * 16 + 9) * spr + 17 and block1[-1] == (1 * 16 + 12) * spr


def test_order_kernel_row_with_two_samples_swapped(ctx):
    t = _synthetic(8, 8, 192, 4)
    t[6, 2, [40, 41]] = t[6, 2, [41, 40]]
    assert t[6, 2, 40] > t[6, 2, 41]
    _check_table(ctx, t, "a row with two samples swapped")                # block 1 runs the whole network, block 0 the merges only
    t = _synthetic(4, 8, 32, 5)[:, :, ::-1].copy()                         # every row descending
    _check_table(ctx, t, "descending rows")


def test_order_kernel_spr_32_and_random_bits(ctx):
    _check_table(ctx, _synthetic(4, 8, 32, 6), "spr = 32")
    _check_table(ctx, _synthetic(5, 24, 32, 7), "spr = 32, a tail row")   # 5 rows: the first 4 are ordered
    bits = np.random.default_rng(8).integers(0, 2 ** 32, size=(4, 8, 96), dtype=np.uint32)
    bits[0, 0, :8] = bits[3, 7, :8]                                        # and a few ties
    _check_table(ctx, bits.view(np.float32), "random bits, spr = 96")
    _check_table(ctx, _synthetic(4, 8, 512, 9), "spr = 512, the largest")


def test_order_kernel_refuses_windows_that_are_not_ordered(native, ctx):
    for shape in ((4, 12, 64), (3, 8, 64), (4, 8, 48), (4, 8, 544)):
        with pytest.raises(native.NerfError):
            ctx.stage_depth_order(np.zeros(shape, np.float32))


# ---- 2. same bits, default against NERF_DEPTH_ORDER=0 -------------------------------------------------------------------------------------
class _Ctx:
    """A counting context (NERF_DEBUG_ZSKIP=1) with `var` unset (the default) or "0".  run() -> (fn's result, [(kernel, executed, total)])."""

    def __init__(self, native, on, var="NERF_DEPTH_ORDER", extra=()):
        self.on = on and not (CONTROL and var == "NERF_DEPTH_ORDER")
        env = [(var, None if self.on else "0"), ("NERF_DEBUG_ZSKIP", "1"), *extra]
        stack = [_env(v, k) for k, v in env]
        for s in stack:
            s.__enter__()
        try:
            self.r = native.Renderer(0)
        finally:
            for s in reversed(stack):
                s.__exit__(None, None, None)
        self.r.load_scene(SCENE)

    def run(self, capfd, fn):
        capfd.readouterr()
        out = fn(self.r)
        return out, [(name, int(e), int(t)) for name, e, t in _LINE.findall(capfd.readouterr().err)]


@pytest.fixture(scope="module")
def pairs(native):
    """(variable, extra environment) -> (switched-off, default) counting contexts on lego"""
    made = {}

    def get(var="NERF_DEPTH_ORDER", extra=()):
        k = (var, tuple(extra))
        if k not in made:
            made[k] = (_Ctx(native, False, var, extra), _Ctx(native, True, var, extra))
        return made[k]

    yield get
    for off, on in made.values():
        off.r.close(); on.r.close()


def _same(capfd, off, on, fn, what, executed=False, skip_empty=False):
    """fn(renderer) in both contexts: every returned array bit for bit, per launch the same kernel and the same total of ReLU k-steps (and,
    where asked, the same executed ones) -> (default's arrays, default's launches, switched-off launches)."""
    a, g_off = off.run(capfd, fn)
    b, g_on = on.run(capfd, fn)
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            if x.dtype == np.uint8:
                assert x.shape == y.shape and np.array_equal(x, y), f"{what}, output {k}: RGBA8 words differ"
            else:
                _eq(y, x, f"{what}, output {k}, default / switched off")
    assert g_on and len(g_on) == len(g_off), (what, g_on, g_off)
    assert {n for n, _, _ in g_on} <= {SIGMA_RAYS, FULL_RAYS} and FULL_RAYS in {n for n, _, _ in g_on}, (what, g_on)
    assert [(n, t) for n, _, t in g_on] == [(n, t) for n, _, t in g_off], f"{what}: kernels or k-step totals differ: {g_on} / {g_off}"
    if executed or skip_empty:
        assert g_on == g_off, f"{what}: executed k-steps differ where the mapping does not: {g_on} / {g_off}"
    return b, g_on, g_off


@pytest.mark.parametrize("window", list(ORDERED) + list(STATIC))
def test_frames_maps_and_rgba8_same_bits(pairs, native, samples, capfd, window):
    off, on = pairs()
    static = window in STATIC
    crop = (ORDERED | STATIC)[window]
    cam = native.camera_from_samples(samples, 800, 800, 64)
    (plain,), _, _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128"), window + " plain", executed=static)
    assert plain.shape == (crop[3], crop[2], 3) and np.isfinite(plain).all()
    aux, _, _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", aux=True), window + " plain + maps", executed=static)
    _eq(aux[0], plain, window + " with maps / without")
    _same(capfd, off, on, lambda r: native.render_image_rgba8(r.coarse, r.fine, cam, 128, seed=0, crop=crop, background=(0.2, 0.4, 0.6),
                                                              alpha="premultiplied"), window + " rgba8", executed=static)
    # skip_empty keeps the static mapping in both contexts: the same frame, the same executed k-steps, the same number of skipped colour heads
    (e_on, st_on), g_on, g_off = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", skip_empty=True, return_stats=True),
                                       window + " skip_empty", skip_empty=True)
    (_, st_off), _ = off.run(capfd, lambda r: _render(native, samples, r, crop, "64+128", skip_empty=True, return_stats=True))
    assert st_on.n_colour_skipped_points == st_off.n_colour_skipped_points, window
    _eq(e_on, plain, window + " skip_empty / plain")
    for counts in ("64+64", "32+0", "20+50"):                              # spr 128; a coarse_only full launch of spr 32; no multiple of 32
        _same(capfd, off, on, lambda r: _render(native, samples, r, crop, counts), f"{window} {counts}", executed=static or counts == "20+50")


def test_ssaa_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    for window in ("8x4", "12x6"):                                        # 16 x 8 and 24 x 12 rays: both ordered on the ray grid
        crop = (ORDERED | STATIC)[window]
        (frame,), _, _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", ssaa=2), f"{window} ssaa 2")
        assert frame.shape == (crop[3], crop[2], 3)


@pytest.mark.parametrize("window,rows", (("24x16", (5, 5, 5, 1)), ("32x8", (4, 4))))
def test_passes_with_tail_rows_and_short_passes(pairs, native, samples, capfd, window, rows):
    """NERF_MAX_RAYS_PER_PASS = 130: the 24 x 16 window in three passes of five rows (four ordered, one tail row behind them) and one of one
    row (not ordered); the 32 x 8 window in two passes of four rows."""
    off, on = pairs(extra=(("NERF_MAX_RAYS_PER_PASS", "130"),))
    whole_off, whole_on = pairs()
    crop = ORDERED[window]
    (frame, st), g, _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", return_stats=True), f"{window} in passes")
    assert st.n_passes == len(rows) and len(g) == 2 * len(rows)
    assert [t for _, _, t in g] == [Z.n_waves(r * crop[2] * spr) * layers * 128 for r in rows for spr, layers in ((64, 7), (192, 8))]
    (whole,), _, _ = _same(capfd, whole_off, whole_on, lambda r: _render(native, samples, r, crop, "64+128"), f"{window} in one pass")
    _eq(frame, whole, f"{window}: passes / one pass")


def test_two_context_multi_frame_same_bits(native, samples, capfd):
    crop = (300, 310, 32, 17)                                              # bands of 9 and 8 rows: one with a tail row
    cam = native.camera_from_samples(samples, 800, 800, 64)
    frames = {}
    for on in (False, True):
        cs = [_Ctx(native, on) for _ in range(2)]
        try:
            frames[on] = native.render_image_multi([c.r for c in cs], cam, 128, gather="host", seed=0, crop=crop, aux=True)
        finally:
            for c in cs:
                c.r.close()
    for k in range(3):
        _eq(frames[True][k], frames[False][k], f"two-context frame, output {k}")
    capfd.readouterr()


# ---- 3. it is really on -------------------------------------------------------------------------------------------------------------------
def test_fine_launch_executes_fewer_ksteps(pairs, native, samples, capfd):
    """lego, 32 x 8 pixels, 64 + 128 samples: the full launch of the default context executes strictly fewer ReLU k-steps than that of the
    switched-off context, and either count lies inside the float64 bracket of zero_skip_cases.py formed over the waves of its own mapping:
    the table nerf_stage_depth_order returns for the pass's t (default) or nerf_debug_wave_tiling's (switched off).  The fine points come
    from the stage calls (render_restatement.py: the same t and the same points as the render's, bit for bit)."""
    off, on = pairs()
    x0, y0, w, h = crop = ORDERED["32x8"]
    _, g_on, g_off = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128"), "lego 32x8")
    cam = native.camera_from_samples(samples, 800, 800, 64)
    re = restate(GpuBackend(native, on.r), cam, 64, 128, crop, 0)
    _eq(re["image"], _render(native, samples, on.r, crop, "64+128"), "restated / rendered")          # the restatement IS this render
    capfd.readouterr()
    pre = Z.preacts_fp64(os.path.join(SCENE, "fine"), re["pts_fine"])[:8]
    ordered = on.r.stage_depth_order(re["t_fine"].reshape(h, w, 192)).astype(np.int32).reshape(-1, 4, 32)
    static = W.table(native, h, w, 192, True, True, True)
    assert ordered.shape == static.shape and (ordered != static).any()
    executed = {}
    for c, g in ((off, g_off), (on, g_on)):
        (name, e, total), = [x for x in g if x[0] == FULL_RAYS]
        live, dead, tot = W.kstep_bracket(ordered if c.on else static, pre, Z.EPS)
        with capfd.disabled():
            print(f"\ndepthorder-count lego 32x8 full launch, depth order {'on' if c.on else 'off'}: executed {e} of {total} ({e / total:.4f});"
                  f" bracket [{live}, {tot - dead}]")
        assert total == tot and live <= e <= tot - dead, (c.on, live, e, tot - dead)
        executed[c is on] = e
    assert executed[True] < executed[False], executed


# ---- 4. tile rotation ---------------------------------------------------------------------------------------------------------------------
def test_rotation_same_bits_and_counts(pairs, native, samples, capfd):
    """NERF_TILE_ROTATION=0 against the default: the rotation changes which workgroup takes a tile and nothing about a tile -- frames, maps,
    executed and total k-steps per launch are the same numbers, ordered or not, skip_empty or not, and for a ray batch and a point batch."""
    off, on = pairs("NERF_TILE_ROTATION")
    for window, crop in (ORDERED | STATIC).items():
        _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", aux=True), f"rotation {window}", executed=True)
    crop = ORDERED["24x16"]
    (_, s_on), _, _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", skip_empty=True, return_stats=True),
                            "rotation 24x16 skip_empty", executed=True)
    (_, s_off), _ = off.run(capfd, lambda r: _render(native, samples, r, crop, "64+128", skip_empty=True, return_stats=True))
    assert s_on.n_colour_skipped_points == s_off.n_colour_skipped_points
    big = (272, 300, 256, 136)                                             # 8704 tiles: 34 rounds of 256 workgroups, 34 different rotations
    _same(capfd, off, on, lambda r: _render(native, samples, r, big, "32+0"), "rotation 256x136 coarse_only", executed=True)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.5, 1.5, size=(3, 40000)).astype(np.float32)       # 313 tiles: a last round that not every workgroup takes part in
    d = rng.normal(size=(40000, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    a = off.r.fine.forward_batch(pts, d); b = on.r.fine.forward_batch(pts, d)
    for name, x, y in zip(("rgb", "sigma"), a, b):
        _eq(y, x, f"rotation forward_batch {name}")
    capfd.readouterr()
