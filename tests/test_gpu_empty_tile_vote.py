"""The empty-tile vote of plain renders (MlpArgs.empty_vote, NERF_EMPTY_TILE_VOTE): every full ray-mode launch of a plain render lets its four
waves vote over the workgroup tile's 128 sigmas behind the alpha head, and a tile without density writes rgb = 0 and skips its colour head.
A sample with sigma = 0 has weight 0 exactly, so nothing of the frame may change.

  1. same bits: a default context against a NERF_EMPTY_TILE_VOTE=0 context in one process -- frames, depth and opacity maps and RGBA8 words
     are compared as uint32 / uint8 on lego at 64 + 128 in every kind of launch that takes the vote (ordered, ordered passes with a tail row and
     a one-row pass, static, coarse_only, SSAA, a caller-supplied ray batch, the two split arithmetics).  Both contexts have
     NERF_DEBUG_EMPTY_TILES=1: the default one must report one voted launch per colour-producing launch with the launch's number of tiles,
     the switched-off one none;
  2. it is really on: with the half-space-empty network (zero_skip_cases.py, case f) on a 16 x 4 window the count the fine launch reports
     equals the number of tiles of nerf_stage_depth_order's table whose 128 entries all have sigma == 0, sigma taken from the stage calls of
     the same context (render_restatement.py: the render's own bits, so there is no float bracket); it lies strictly between 0 and 96, is 0
     when switched off, and is 0 in a NERF_DEBUG_ZSKIP=1 context, whose k-step counters are those of a switched-off context (the k-step
     diagnostic describes the dense colour head);
  3. the opt-in is untouched: skip_empty=True renders the same frame, skips the same number of colour heads and counts the same k-steps in a
     default and in a switched-off context, and is no voted launch."""
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
import zero_skip_cases as Z  # noqa: E402
from render_restatement import GpuBackend, restate  # noqa: E402
from test_gpu_ray_grouping import FULL_RAYS, _LINE, _eq, _load, _render  # noqa: E402  (its helpers, not its tests)
from test_gpu_zero_skip import _env  # noqa: E402

pytestmark = pytest.mark.gpu

VAR = "NERF_EMPTY_TILE_VOTE"
_VOTE = re.compile(r"nerf empty tiles: (\S+) tiles_skipped=(\d+) tiles=(\d+)")
KERNEL = {"f32": FULL_RAYS, "bf16x3": "nerf_mlp_kernel_bf16x3<full,rays>", "f16x2": "nerf_mlp_kernel_f16x2<full,rays>"}
# all at (300, 310) of the 800 x 800 view, across the model's edge, as the depth-ordering tests
WINDOWS = {"32x8": (300, 310, 32, 8), "24x16": (300, 310, 24, 16), "12x6": (300, 310, 12, 6), "8x4": (300, 310, 8, 4)}
F_WINDOW = (388, 404, 16, 4)   # case f: the rows around ray_grouping_cases.F_ROW_WINDOW -- two 8 x 4 blocks, 64 rays x 192 samples = 96 tiles


def _tiles(n_points):
    return (n_points + 127) // 128


class _Ctx:
    """A context that reports its voted launches (NERF_DEBUG_EMPTY_TILES=1), with the vote on (the variable unset: the default) or "0", and
    with or without the k-step diagnostic.  run() -> (fn's result, [(kernel, tiles skipped, tiles)], [(kernel, executed, total)])."""

    def __init__(self, native, vote, zskip=False, extra=()):
        env = [(VAR, None if vote else "0"), ("NERF_DEBUG_EMPTY_TILES", "1"), ("NERF_DEBUG_ZSKIP", "1" if zskip else None), *extra]
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
        err = capfd.readouterr().err
        return out, [(n, int(s), int(t)) for n, s, t in _VOTE.findall(err)], [(n, int(e), int(t)) for n, e, t in _LINE.findall(err)]


@pytest.fixture(scope="module")
def pairs(native):
    """(scene, k-step diagnostic, extra environment) -> (switched-off, default) contexts"""
    made = {}

    def get(scene=SCENE, zskip=False, extra=()):
        k = (scene, zskip, tuple(extra))
        if k not in made:
            made[k] = (_Ctx(native, False, zskip, extra), _Ctx(native, True, zskip, extra))
            for c in made[k]:
                _load(native, c, scene)
        return made[k]

    yield get
    for off, on in made.values():
        off.r.close(); on.r.close()


def _same(capfd, off, on, fn, what, kernel, tiles):
    """fn(renderer) in both contexts: every returned array bit for bit; the default context voted in exactly the launches `tiles` lists (their
    numbers of workgroup tiles, in order), the switched-off context in none -> (default's arrays, default's voted launches)."""
    a, v_off, _ = off.run(capfd, fn)
    b, v_on, _ = on.run(capfd, fn)
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            if x.dtype == np.uint8:
                assert x.shape == y.shape and np.array_equal(x, y), f"{what}, output {k}: RGBA8 words differ"
            else:
                _eq(y, x, f"{what}, output {k}, default / switched off")
    assert v_off == [], f"{what}: the switched-off context voted: {v_off}"
    assert [(n, t) for n, _, t in v_on] == [(kernel, t) for t in tiles], f"{what}: voted launches {v_on}, expected tiles {tiles}"
    assert all(0 <= s <= t for _, s, t in v_on), (what, v_on)
    return b, v_on


def _frame_maps_rgba8(native, samples, capfd, off, on, crop, counts, what, tiles, dtype="f32", **kw):
    cam = native.camera_from_samples(samples, 800, 800, int(counts.split("+")[0]))
    nf, coarse_only = int(counts.split("+")[1]), counts.endswith("+0")
    aux, v = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, counts, aux=True, dtype=dtype, **kw), what + " frame + maps",
                   KERNEL[dtype], tiles)
    assert aux[0].shape == (crop[3], crop[2], 3) and np.isfinite(aux[0]).all() and aux[1].shape == aux[2].shape == (crop[3], crop[2])
    _same(capfd, off, on, lambda r: native.render_image_rgba8(r.coarse, r.fine, cam, nf, seed=0, crop=crop, coarse_only=coarse_only, dtype=dtype,
                                                              background=(0.2, 0.4, 0.6), alpha="premultiplied", **kw), what + " rgba8",
          KERNEL[dtype], tiles)
    return aux, v


# ---- 1. same bits -------------------------------------------------------------------------------------------------------------------------
def test_ordered_window_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _, v = _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["32x8"], "64+128", "32x8 ordered", [384])   # 8 blocks of 48 tiles
    assert 0 < v[0][1] < 384, v                                            # the window lies across the model's edge: some slabs are empty, not all


def test_ordered_passes_with_tail_row_and_one_row_pass_same_bits(pairs, native, samples, capfd):
    """NERF_MAX_RAYS_PER_PASS = 130: the 24 x 16 window in three passes of five rows (four ordered, one tail row behind them) and one of one row."""
    off, on = pairs(extra=(("NERF_MAX_RAYS_PER_PASS", "130"),))
    tiles = [_tiles(rows * 24 * 192) for rows in (5, 5, 5, 1)]
    aux, _ = _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["24x16"], "64+128", "24x16 in passes", tiles)
    whole_off, whole_on = pairs()
    whole, _ = _same(capfd, whole_off, whole_on, lambda r: _render(native, samples, r, WINDOWS["24x16"], "64+128", aux=True), "24x16 in one pass",
                     FULL_RAYS, [_tiles(16 * 24 * 192)])
    for k in range(3):
        _eq(aux[k], whole[k], f"24x16: passes / one pass, output {k}")


def test_static_window_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["12x6"], "64+128", "12x6 static", [_tiles(72 * 192)])   # row width no multiple of 8


def test_coarse_only_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["32x8"], "32+0", "32x8 coarse_only", [_tiles(256 * 32)])


def test_ssaa_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["8x4"], "64+128", "8x4 ssaa 2", [_tiles(16 * 8 * 192)], ssaa=2)


def test_caller_supplied_ray_batch_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    rng = np.random.default_rng(64)
    origin = np.float32(samples["camera_origin"])
    dirs = (rng.uniform(-1.0, 1.0, size=(64, 3)) - origin).astype(np.float32)
    call = lambda r: native.render_rays(r.coarse, r.fine, origin, dirs, float(samples["near"]), float(samples["far"]), 128, seed=0, aux=True)
    out, _ = _same(capfd, off, on, call, "64-ray batch", FULL_RAYS, [_tiles(64 * 192)])
    assert out[0].shape == (64, 3) and np.isfinite(out[0]).all() and out[0].std() > 0


@pytest.mark.parametrize("dtype", ("bf16x3", "f16x2"))
def test_split_arithmetics_same_bits(pairs, native, samples, capfd, dtype):
    off, on = pairs()
    _frame_maps_rgba8(native, samples, capfd, off, on, WINDOWS["32x8"], "64+128", f"32x8 {dtype}", [384], dtype=dtype)


# ---- 2. it is really on -------------------------------------------------------------------------------------------------------------------
def test_vote_skips_the_tiles_without_density(pairs, native, oracle, samples, capfd, tmp_path):
    d = Z._make_case("f", write_random_net(tmp_path / "net", 20240), tmp_path, oracle)[0]
    x0, y0, w, h = crop = F_WINDOW
    off, on = pairs(d)
    zs_off, zs_on = pairs(d, zskip=True)
    render = lambda r: _render(native, samples, r, crop, "64+128")
    (frame,), v_on = _same(capfd, off, on, render, "case f 16x4", FULL_RAYS, [96])
    assert (frame != 1.0).any()                                            # some ray does meet density
    # what the vote must have found, from the context's own stage calls: the render's sigma bits at the slots of the launch's order table
    cam = native.camera_from_samples(samples, 800, 800, 64)
    re_ = restate(GpuBackend(native, on.r), cam, 64, 128, crop, 0)
    _eq(re_["image"], frame, "restated / rendered")                        # the restatement IS this render
    table = on.r.stage_depth_order(re_["t_fine"].reshape(h, w, 192)).astype(np.int64)
    assert table.shape == (96 * 128,)                                      # all four rows are ordered: the launch has no static part
    sigma = np.ascontiguousarray(re_["sigma_fine"], dtype=np.float32).reshape(-1)
    assert (sigma >= 0).all()
    want = int((sigma[table].reshape(96, 128) == 0).all(axis=1).sum())
    capfd.readouterr()
    with capfd.disabled():
        print(f"\nemptyvote-count case f {crop}: tiles skipped {v_on[0][1]} of {v_on[0][2]}, all-zero tiles of the order table {want}")
    assert v_on[0][1] == want and 0 < want < 96, (v_on, want)
    # the k-step diagnostic switches the vote off: no voted launch, and the counters of a switched-off context
    (z_frame,), z_votes, z_on = zs_on.run(capfd, lambda r: (render(r),))
    (_,), z_votes_off, z_off = zs_off.run(capfd, lambda r: (render(r),))
    assert z_votes == [] and z_votes_off == [], (z_votes, z_votes_off)
    assert z_on and z_on == z_off and FULL_RAYS in {n for n, _, _ in z_on}, (z_on, z_off)
    assert [t for n, _, t in z_on if n == FULL_RAYS] == [Z.n_waves(64 * 192) * 8 * 128], z_on   # the dense colour head: all eight ReLU layers of every wave
    _eq(z_frame, frame, "case f, k-step diagnostic on / default")


# ---- 3. the opt-in is untouched -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ("32x8", "12x6"))
def test_skip_empty_is_untouched(pairs, native, samples, capfd, window):
    crop = WINDOWS[window]
    render = lambda r: _render(native, samples, r, crop, "64+128", skip_empty=True, return_stats=True)
    off, on = pairs()
    (frame, st_on), _ = _same(capfd, off, on, render, window + " skip_empty", FULL_RAYS, [])        # no voted launch: skip_empty's own switch
    (_, st_off), _, _ = off.run(capfd, render)
    assert st_on.n_colour_skipped_points == st_off.n_colour_skipped_points > 0, (st_on.n_colour_skipped_points, st_off.n_colour_skipped_points)
    (plain, st_plain), _ = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, "64+128", return_stats=True), window + " plain",
                                 FULL_RAYS, [_tiles(crop[2] * crop[3] * 192)])
    assert st_plain.n_colour_skipped_points == 0                           # plain renders keep reporting none
    _eq(frame, plain, window + " skip_empty / plain")
    zs_off, zs_on = pairs(zskip=True)
    (z_frame, z_st), _, g_on = zs_on.run(capfd, render)
    (_, _), _, g_off = zs_off.run(capfd, render)
    assert g_on and g_on == g_off, f"{window} skip_empty: k-step counters differ: {g_on} / {g_off}"
    assert z_st.n_colour_skipped_points == st_on.n_colour_skipped_points
    _eq(z_frame, frame, window + " skip_empty, k-step diagnostic on / off")
