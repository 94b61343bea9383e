"""The fine cut of plain renders (MlpArgs.fine_cut, NERF_FINE_CUT): the depth-ordered full f32 launch whose densities and colours go to the
compositor alone walks the ordered tiles of an 8 x 4 pixel block front to back, keeps every ray's transmittance as k_composite will compute
it, and leaves the block once all 32 rays are behind the reference's T < 1e-4 cut.  The compositor gives a sample behind the cut the weight 0
whatever its density and colour, so nothing of the frame may change.

  1. same bits: a NERF_FINE_CUT=2 context against a NERF_FINE_CUT=0 context in one process -- frames, depth and opacity maps are compared as
     uint32 on lego crops of the bench view that hold object, background and silhouette, in every kind of render.  Both contexts have
     NERF_DEBUG_FINE_CUT=1: the first one must report exactly the launches that qualify, with their tiles and blocks, the other none.  The
     coarse network's ordered full launch of a coarse_only render qualifies by the same rule (its outputs go to the compositor alone) and is cut;
  2. the counter: tiles_skipped of the first crop lies in a bracket built from the stage calls' fine sigma and t and the order table, with T in
     float32 on the host (the host's expf is not the device's: a ray whose T comes within a relative 1e-3 of 1e-4 counts as cut there for the
     upper bound and as not cut there for the lower one), and is above 0;
  3. two synthetic networks through the tensor loader: the all-zero network cuts nothing (0 tiles, opacity 0); a fog (alpha bias 1e4) is opaque
     and cut, inside the same host bracket;
  4. the order kernel's per-block flags on ascending rows with ties, one swapped pair, and a NaN;
  5. a NERF_DEBUG_ZSKIP=1 context runs without the cut: no cut launch, and the fine launch's k-step totals are those of every sample;
  6. a cut launch hands out whole blocks, so by default only launches of at least 48 blocks per workgroup are cut; groups 1 to 5 run in
     NERF_FINE_CUT=2 contexts, which cut every qualifying launch.  A default context must cut no small window and must cut a launch of 48
     blocks per workgroup, with the same bits."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import SCENE

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "tools"))
import zero_skip_cases as Z  # noqa: E402
from render_restatement import GpuBackend, restate  # noqa: E402
from test_gpu_coarse_cut import FIRST, WINDOWS, _load_tensors, _render, _tiles  # noqa: E402  (its helpers, not its tests)
from test_gpu_ray_grouping import FULL_RAYS, _LINE, _eq  # noqa: E402
from test_gpu_zero_skip import _env  # noqa: E402

pytestmark = pytest.mark.gpu

VAR = "NERF_FINE_CUT"
MIN_BLOCKS_PER_WORKGROUP = 48                                                  # nerf_internal.h kFineCutMinBlocksPerWorkgroup
_CUT = re.compile(r"nerf fine cut: (\S+) tiles_skipped=(\d+) tiles=(\d+) blocks=(\d+)")


def _launch(w, h, spr):
    """(tiles, blocks) of the ordered full launch of w x h rays, spr samples each"""
    return _tiles(w * h * spr), (w // 8) * (h // 4)


class _Ctx:
    """A context that reports its fine-cut launches (NERF_DEBUG_FINE_CUT=1), with the cut on for every qualifying launch (cut = True: "2"),
    off ("0"), or as it comes (None: the variable unset).  run() -> (fn's result, [(tiles skipped, tiles, blocks)], [(kernel, executed, total)])."""

    def __init__(self, native, cut, zskip=False, extra=()):
        env = [(VAR, {True: "2", False: "0", None: None}[cut]), ("NERF_DEBUG_FINE_CUT", "1"), ("NERF_DEBUG_ZSKIP", "1" if zskip else None), *extra]
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
        cuts = _CUT.findall(err)
        assert all(n == FULL_RAYS for n, _, _, _ in cuts), cuts
        return out, [(int(s), int(t), int(b)) for _, s, t, b in cuts], [(n, int(e), int(t)) for n, e, t in _LINE.findall(err)]


@pytest.fixture(scope="module")
def pairs(native):
    """(k-step diagnostic, extra environment) -> (switched-off, NERF_FINE_CUT=2) contexts with the lego scene"""
    made = {}

    def get(zskip=False, extra=(), load=True):
        k = (zskip, tuple(extra), load)
        if k not in made:
            made[k] = (_Ctx(native, False, zskip, extra), _Ctx(native, True, zskip, extra))
            if load:
                for c in made[k]:
                    c.r.load_scene(SCENE)
        return made[k]

    yield get
    for off, on in made.values():
        off.r.close(); on.r.close()


def _same(capfd, off, on, fn, what, launches, spr=192):
    """fn(renderer) in both contexts: every returned array bit for bit; the cutting context cut in exactly the launches `launches` lists
    ((tiles, blocks), in order), the switched-off context in none -> (cutting context's arrays, its cut launches)."""
    a, c_off, _ = off.run(capfd, fn)
    b, c_on, _ = on.run(capfd, fn)
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            _eq(y, x, f"{what}, output {k}, cut / switched off")
    assert c_off == [], f"{what}: the switched-off context cut: {c_off}"
    assert [(t, n) for _, t, n in c_on] == list(launches), f"{what}: cut launches {c_on}, expected (tiles, blocks) {launches}"
    assert all(0 <= s <= n * (spr // 4 - 1) for s, t, n in c_on), (what, c_on)  # a block's first tile is always evaluated
    return b, c_on


def _window(native, samples, capfd, off, on, window, launches, what=None, nc=64, nf=128, spr=None, **kw):
    crop = WINDOWS[window]
    out, cuts = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, nc, nf, **kw), what or window, launches, spr or nc + nf)
    assert out[0].shape == (crop[3], crop[2], 3) and np.isfinite(out[0]).all() and out[1].shape == out[2].shape == (crop[3], crop[2])
    return out, cuts


# ---- 1. same bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,launch", [("32x8", _launch(32, 8, 192)), ("8x4", _launch(8, 4, 192)), ("24x12", _launch(24, 12, 192)),
                                           ("32x10", _launch(32, 10, 192))])
def test_windows_same_bits(pairs, native, samples, capfd, window, launch):
    """32 x 8; one block (fewer blocks than workgroups); nine blocks (no multiple of 4); two tail rows behind the blocks (units of one tile)."""
    off, on = pairs()
    out, cuts = _window(native, samples, capfd, off, on, window, [launch])
    assert cuts[0][0] > 0, cuts                                               # each of these windows holds a block that lies on the model
    if window in ("32x8", "32x10"):
        assert (out[2] > 0.99).any() and (out[2] < 0.01).any()                # object and background


def test_width_no_multiple_of_8_does_not_qualify(pairs, native, samples, capfd):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "28x8", [])                      # no 8 x 4 pixel blocks, no order table


def test_passes_with_a_one_row_last_pass_same_bits(pairs, native, samples, capfd):
    """NERF_MAX_RAYS_PER_PASS = 100: the 24 x 9 window in two passes of four rows (three blocks each) and one of one row, which does not qualify."""
    off, on = pairs(extra=(("NERF_MAX_RAYS_PER_PASS", "100"),))
    out, _ = _window(native, samples, capfd, off, on, "24x9", [_launch(24, 4, 192)] * 2, "24x9 in passes")
    whole_off, whole_on = pairs()
    whole, _ = _window(native, samples, capfd, whole_off, whole_on, "24x9", [_launch(24, 9, 192)], "24x9 in one pass")
    for k in range(3):
        _eq(out[k], whole[k], f"24x9: passes / one pass, output {k}")


def test_ssaa_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "8x4", [_launch(16, 8, 192)], "8x4 ssaa 2", ssaa=2)


@pytest.mark.parametrize("nc,nf,qualifies", [(8, 16, False), (62, 128, False), (32, 64, True), (96, 32, True)])
def test_sample_counts_same_bits(pairs, native, samples, capfd, nc, nf, qualifies):
    """24 and 190 samples per ray are no multiple of 32: no order table, no cut; 96 and 128 have blocks of 24 and 32 tiles."""
    off, on = pairs()
    _, cuts = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, nc + nf)] if qualifies else [], f"32x8 {nc}+{nf}", nc=nc, nf=nf)
    if qualifies:
        assert cuts[0][0] > 0, cuts


@pytest.mark.parametrize("dtype", ("bf16x3", "f16x2"))
def test_split_arithmetics_have_no_fine_cut(pairs, native, samples, capfd, dtype):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "32x8", [], f"32x8 {dtype}", dtype=dtype)


@pytest.mark.parametrize("mode,launches", [("coarse_only", [_launch(32, 8, 64)]), ("skip_empty", []), ("skip_dead", []), ("certify_zero", [])])
def test_other_render_modes_same_bits(pairs, native, samples, capfd, mode, launches):
    """By the rule -- the ordered full f32 ray-mode launch of a plain image render whose sigma and rgb go to the compositor and nowhere else:
    coarse_only composites the coarse network's ordered full launch, which is cut; a skip_empty launch keeps the static mapping (no table);
    skip_dead and certify_zero have their own launches."""
    off, on = pairs()
    plain, _ = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 192)], "32x8 plain")
    coarse_only = mode == "coarse_only"
    out, _ = _window(native, samples, capfd, off, on, "32x8", launches, f"32x8 {mode}", nf=0 if coarse_only else 128, spr=64 if coarse_only else 192,
                     **{mode: True})
    if not coarse_only:
        for k in range(3):
            _eq(out[k], plain[k], f"32x8 {mode} / plain, output {k}")


def test_caller_supplied_ray_batch_is_not_cut(pairs, native, samples, capfd):
    off, on = pairs()
    rng = np.random.default_rng(64)
    origin = np.float32(samples["camera_origin"])
    dirs = (rng.uniform(-1.0, 1.0, size=(256, 3)) - origin).astype(np.float32)
    call = lambda r: native.render_rays(r.coarse, r.fine, origin, dirs, float(samples["near"]), float(samples["far"]), 128, seed=0, aux=True)
    out, _ = _same(capfd, off, on, call, "256-ray batch", [])
    assert out[0].shape == (256, 3) and np.isfinite(out[0]).all() and out[0].std() > 0


# ---- 2. the counter -----------------------------------------------------------------------------------------------------------------------
def _skipped(table, sigma, t, far, w, h, threshold):
    """tiles the walk leaves out on an h x w window (rays row-major; table: the window's order table) when a ray counts as cut behind the first
    sample with T < threshold; T walks in float32.  A block is left behind the tile that holds the sample which cuts its last ray."""
    n = t.shape[1]
    delta = np.maximum(np.concatenate([t[:, 1:], np.full((len(t), 1), far, np.float32)], axis=1) - t, np.float32(0))
    alpha = np.float32(1) - np.exp(-sigma * delta, dtype=np.float32)
    T = np.ones(len(t), np.float32)
    cutting = np.full(len(t), -1)                                               # index of the sample that cuts the ray; -1: never cut
    for i in range(n):
        live = cutting < 0
        T = np.where(live, T * (np.float32(1) - alpha[:, i]), T).astype(np.float32)
        cutting[live & (T < np.float32(threshold))] = i
    position = np.empty(len(t) * n, np.int64)                                   # slot -> position in the table
    position[table.astype(np.int64)] = np.arange(table.size)
    block_tiles, skipped = n // 4, 0
    for b in range((h // 4) * (w // 8)):
        by, bx = divmod(b, w // 8)
        rays = ((4 * by + np.arange(4))[:, None] * w + 8 * bx + np.arange(8)[None, :]).reshape(-1)
        if (cutting[rays] < 0).any():
            continue
        last = (position[rays * n + cutting[rays]] // 128).max()               # tile (of the launch) in which the block's last ray is cut
        skipped += (b + 1) * block_tiles - 1 - int(last)
    return skipped


def _bracket(native, ctx, samples, crop, nc=64, nf=128):
    x0, y0, w, h = crop
    cam = native.camera_from_samples(samples, 800, 800, nc)
    re_ = restate(GpuBackend(native, ctx.r), cam, nc, nf, crop, 0)
    sigma, t = np.asarray(re_["sigma_fine"], np.float32), np.asarray(re_["t_fine"], np.float32)
    table = ctx.r.stage_depth_order(t.reshape(h, w, -1))
    assert ctx.r.stage_depth_order_flags(t.reshape(h, w, -1)).all()             # the resampler's rows ascend
    far = np.float32(cam.far)
    return (_skipped(table, sigma, t, far, w, h, 1e-4 * (1 - 1e-3)),            # a ray that comes that close is not cut there ...
            _skipped(table, sigma, t, far, w, h, 1e-4 * (1 + 1e-3)))            # ... or is


def test_tiles_skipped_lies_in_the_host_bracket(pairs, native, samples, capfd):
    off, on = pairs()
    _, cuts = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 192)])
    lo, hi = _bracket(native, on, samples, FIRST)
    capfd.readouterr()
    with capfd.disabled():
        print(f"\nfinecut-count {FIRST}: tiles skipped {cuts[0][0]} of {cuts[0][1]} in {cuts[0][2]} blocks, host bracket [{lo}, {hi}]")
    assert lo <= cuts[0][0] <= hi and cuts[0][0] > 0, (cuts, lo, hi)


# ---- 3. synthetic networks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_bias,fog", [(1e4, True), (0.0, False)])
def test_fog_is_cut_and_nothing_cuts_nothing(pairs, native, samples, capfd, alpha_bias, fog):
    off, on = pairs(load=False)
    for c in (off, on):
        _load_tensors(native, c.r, alpha_bias)
    out, cuts = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 192)], f"32x8 alpha bias {alpha_bias}")
    if not fog:
        assert cuts[0][0] == 0 and (out[2] == 0.0).all(), cuts                 # nothing at all
        return
    assert (out[2] >= 0.999).all() and cuts[0][0] > 0, cuts                    # opaque fog
    # not blocks x (tiles - 1): the fine samples of a fog cluster together and some deltas are tiny -- the host's walk says how many
    lo, hi = _bracket(native, on, samples, FIRST)
    capfd.readouterr()
    with capfd.disabled():
        print(f"\nfinecut-fog {FIRST}: tiles skipped {cuts[0][0]} of {cuts[0][1]} in {cuts[0][2]} blocks, host bracket [{lo}, {hi}]")
    assert lo <= cuts[0][0] <= hi, (cuts, lo, hi)


# ---- 4. the order kernel's flags ----------------------------------------------------------------------------------------------------------
def _keys_ascend(t):
    """per block of t (rows, rw, spr): every row's keys (uint32 bits of t) << 32 | ray-in-block * spr + sample ascend with the sample index"""
    rows, rw, spr = t.shape
    bits = np.ascontiguousarray(t, np.float32).view(np.uint32).astype(np.uint64)
    out = []
    for by in range(rows // 4):
        for bx in range(rw // 8):
            blk = bits[4 * by:4 * by + 4, 8 * bx:8 * bx + 8].reshape(32, spr)
            key = (blk << np.uint64(32)) | (np.arange(32, dtype=np.uint64)[:, None] * np.uint64(spr) + np.arange(spr, dtype=np.uint64)[None, :])
            out.append(int((key[:, 1:] > key[:, :-1]).all()))
    return np.array(out, np.uint32)


def test_order_flags(pairs):
    _, on = pairs()
    rng = np.random.default_rng(5)
    rows, rw, spr = 8, 24, 64                                                   # six blocks; rows ascending with ties, the same t on every ray
    base = np.sort(rng.uniform(2.0, 6.0, spr).astype(np.float32))
    base[10] = base[9]; base[40:44] = base[40]
    t = np.ascontiguousarray(np.broadcast_to(base, (rows, rw, spr)))
    assert np.array_equal(on.r.stage_depth_order_flags(t), np.ones(6, np.uint32))
    swapped = t.copy()
    swapped[5, 9, 20], swapped[5, 9, 21] = t[5, 9, 21], t[5, 9, 20]             # row 5, column 9: block (1, 1) = 4
    assert swapped[5, 9, 20] > swapped[5, 9, 21]
    want = np.ones(6, np.uint32); want[4] = 0
    assert np.array_equal(on.r.stage_depth_order_flags(swapped), want)
    nan = t.copy()
    nan[2, 17, 30] = np.nan                                                     # block (0, 2): a NaN's bits lie above every finite t's
    flags = on.r.stage_depth_order_flags(nan)
    assert np.array_equal(flags, _keys_ascend(nan)) and flags[2] == 0 and flags.sum() == 5, flags
    assert np.array_equal(_keys_ascend(t), np.ones(6, np.uint32)) and np.array_equal(_keys_ascend(swapped), want)


# ---- 5. the k-step diagnostic runs without the cut ----------------------------------------------------------------------------------------
def test_zskip_context_counts_every_sample(pairs, native, samples, capfd):
    zs_off, zs_on = pairs(zskip=True)
    off, on = pairs()
    render = lambda r: _render(native, samples, r, FIRST)
    a, c_on, g_on = zs_on.run(capfd, render)
    b, c_off, g_off = zs_off.run(capfd, render)
    assert c_on == [] and c_off == [], (c_on, c_off)
    assert g_on and g_on == g_off, (g_on, g_off)
    assert [t for n, _, t in g_on if n == FULL_RAYS] == [Z.n_waves(32 * 8 * 192) * 8 * 128], g_on     # eight ReLU layers of every wave of every sample
    plain, _ = _same(capfd, off, on, render, "32x8 plain", [_launch(32, 8, 192)])
    for k in range(3):
        _eq(a[k], plain[k], f"k-step diagnostic on / cut, output {k}")
        _eq(b[k], plain[k], f"k-step diagnostic on, switched off / cut, output {k}")


# ---- 6. the default asks for 48 blocks per workgroup --------------------------------------------------------------------------------------
def test_default_context_cuts_large_launches_only(pairs, native, samples, capfd):
    off, _ = pairs()
    ctx = _Ctx(native, None)
    try:
        ctx.r.load_scene(SCENE)
        n_cus = ctx.r.device_info()["n_cus"]
        _window(native, samples, capfd, off, ctx, "32x8", [], "32x8 default context")          # 8 blocks: static walk
        rows = 4 * -(-MIN_BLOCKS_PER_WORKGROUP * n_cus // 100)                                 # 100 blocks per block row of the 800-pixel view
        assert rows <= 800
        y0 = (800 - rows) // 2 // 4 * 4
        crop = (0, y0, 800, rows)
        out, cuts = _same(capfd, off, ctx, lambda r: _render(native, samples, r, crop), "48 blocks per workgroup", [_launch(800, rows, 192)])
        assert cuts[0][0] > 0 and (out[2] > 0.99).any() and (out[2] < 0.01).any(), cuts
        below = (0, y0, 800, rows - 4)
        _same(capfd, off, ctx, lambda r: _render(native, samples, r, below), "one block row short of 48 blocks per workgroup", [])
    finally:
        ctx.r.close()
