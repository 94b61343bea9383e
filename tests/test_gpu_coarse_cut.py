"""The coarse cut of plain renders (MlpArgs.ray_cut, NERF_COARSE_CUT): the f32 sampling launch walks the samples of an 8 x 4 pixel block front to
back, keeps every ray's transmittance as the resampler will compute it, and leaves the block once all 32 rays are behind the reference's
T < 1e-4 cut.  The resampler gives a sample behind the cut the weight 0 whatever its density, so nothing of the frame may change.

  1. same bits: a NERF_COARSE_CUT=2 context against a NERF_COARSE_CUT=0 context in one process -- frames, depth and opacity maps are compared as uint32 on
     lego crops of the bench view that hold object, background and silhouette, in every kind of render.  Both contexts have
     NERF_DEBUG_COARSE_CUT=1: the first one must report exactly the launches that qualify, with their tiles and blocks, the other none;
  2. the counter: tiles_skipped of the first crop lies in a bracket built from the stage calls' coarse sigma and t with T in float32 on the
     host (the host's expf is not the device's: a ray whose T comes within a relative 1e-3 of 1e-4 counts as cut there for the upper bound and
     as not cut there for the lower one), and is above 0;
  3. two synthetic networks through the tensor loader: a fog (all weights zero, alpha bias 1e4) cuts every ray behind its first sample, so every
     block leaves after its first tile: tiles_skipped = blocks x (spr / 4 - 1) exactly; the all-zero network cuts nothing: 0;
  4. a NERF_DEBUG_ZSKIP=1 context runs without the cut: no cut launch, and the sampling launch's k-step totals are those of every sample;
  5. a cut launch hands out whole blocks, so by default only launches of at least 16 blocks per workgroup are cut (a smaller one would leave
     workgroups idle); groups 1 to 4 run in NERF_COARSE_CUT=2 contexts, which cut every qualifying launch.  A default context must cut no
     small window and must cut a launch of 16 blocks per workgroup, with the same bits."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import SHAPES

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "tools"))
import zero_skip_cases as Z  # noqa: E402
from render_restatement import GpuBackend, restate  # noqa: E402
from test_gpu_ray_grouping import SIGMA_RAYS, _LINE, _eq  # noqa: E402  (its helpers, not its tests)
from test_gpu_zero_skip import _env  # noqa: E402

pytestmark = pytest.mark.gpu

VAR = "NERF_COARSE_CUT"
_CUT = re.compile(r"nerf coarse cut: (\S+) tiles_skipped=(\d+) tiles=(\d+) blocks=(\d+)")
# 8 x 4 pixel blocks of the 800 x 800 view from (312, 304): the two left columns of blocks see background and the model's edge (no block of them
# is cut as a whole), the two right ones lie on the model (tools/coarse_cut_model.py's walk on the oracle's densities: cut behind sample 22 .. 32)
FIRST = (312, 304, 32, 8)
WINDOWS = {"32x8": FIRST, "8x4": (336, 304, 8, 4), "24x12": (320, 304, 24, 12), "32x10": (312, 304, 32, 10), "28x8": (312, 304, 28, 8),
           "24x9": (320, 304, 24, 9)}


def _tiles(n_points):
    return (n_points + 127) // 128


def _launch(w, h, nc):
    """(tiles, blocks) of the sampling launch of w x h rays, nc samples each"""
    return _tiles(w * h * nc), (w // 8) * (h // 4)


class _Ctx:
    """A context that reports its cut launches (NERF_DEBUG_COARSE_CUT=1), with the cut on for every qualifying launch ("2"; cut = None: the
    variable unset, the default, which asks for 16 blocks per workgroup) or "0", and with or
    without the k-step diagnostic.  run() -> (fn's result, [(tiles skipped, tiles, blocks)], [(kernel, executed, total)])."""

    def __init__(self, native, cut, zskip=False, extra=()):
        env = [(VAR, {True: "2", False: "0", None: None}[cut]), ("NERF_DEBUG_COARSE_CUT", "1"), ("NERF_DEBUG_ZSKIP", "1" if zskip else None), *extra]
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
        assert all(n == SIGMA_RAYS for n, _, _, _ in cuts), cuts
        return out, [(int(s), int(t), int(b)) for _, s, t, b in cuts], [(n, int(e), int(t)) for n, e, t in _LINE.findall(err)]


@pytest.fixture(scope="module")
def pairs(native):
    """(k-step diagnostic, extra environment) -> (switched-off, NERF_COARSE_CUT=2) contexts with the lego scene"""
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


def _same(capfd, off, on, fn, what, launches):
    """fn(renderer) in both contexts: every returned array bit for bit; the default context cut in exactly the launches `launches` lists
    ((tiles, blocks), in order), the switched-off context in none -> (default's arrays, default's cut launches)."""
    a, c_off, _ = off.run(capfd, fn)
    b, c_on, _ = on.run(capfd, fn)
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            _eq(y, x, f"{what}, output {k}, default / switched off")
    assert c_off == [], f"{what}: the switched-off context cut: {c_off}"
    assert [(t, n) for _, t, n in c_on] == list(launches), f"{what}: cut launches {c_on}, expected (tiles, blocks) {launches}"
    assert all(0 <= s <= t - n for s, t, n in c_on), (what, c_on)           # a block's first tile is always evaluated
    return b, c_on


def _render(native, samples, r, crop, nc=64, nf=128, **kw):
    cam = native.camera_from_samples(samples, 800, 800, nc)
    return native.render_image(r.coarse, r.fine, cam, nf, seed=0, crop=crop, aux=True, **kw)


def _window(native, samples, capfd, off, on, window, launches, what=None, nc=64, nf=128, **kw):
    crop = WINDOWS[window]
    out, cuts = _same(capfd, off, on, lambda r: _render(native, samples, r, crop, nc, nf, **kw), what or window, launches)
    assert out[0].shape == (crop[3], crop[2], 3) and np.isfinite(out[0]).all() and out[1].shape == out[2].shape == (crop[3], crop[2])
    return out, cuts


# ---- 1. same bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,launch", [("32x8", _launch(32, 8, 64)), ("8x4", _launch(8, 4, 64)), ("24x12", _launch(24, 12, 64)),
                                           ("32x10", _launch(32, 10, 64))])
def test_windows_same_bits(pairs, native, samples, capfd, window, launch):
    """32 x 8; one block (fewer blocks than workgroups); nine blocks (no multiple of 4); two tail rows behind the blocks (units of one tile)."""
    off, on = pairs()
    out, cuts = _window(native, samples, capfd, off, on, window, [launch])
    assert cuts[0][0] > 0, cuts                                               # each of these windows holds a block that lies on the model
    if window in ("32x8", "32x10"):
        assert (out[2] > 0.99).any() and (out[2] < 0.01).any()                # object and background


def test_width_no_multiple_of_8_does_not_qualify(pairs, native, samples, capfd):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "28x8", [])                      # the sampling launch is tiled 4 x 4 x 2 there


def test_passes_with_a_one_row_last_pass_same_bits(pairs, native, samples, capfd):
    """NERF_MAX_RAYS_PER_PASS = 100: the 24 x 9 window in two passes of four rows (three blocks each) and one of one row, which does not qualify."""
    off, on = pairs(extra=(("NERF_MAX_RAYS_PER_PASS", "100"),))
    out, _ = _window(native, samples, capfd, off, on, "24x9", [_launch(24, 4, 64)] * 2, "24x9 in passes")
    whole_off, whole_on = pairs()
    whole, _ = _window(native, samples, capfd, whole_off, whole_on, "24x9", [_launch(24, 9, 64)], "24x9 in one pass")
    for k in range(3):
        _eq(out[k], whole[k], f"24x9: passes / one pass, output {k}")


def test_ssaa_same_bits(pairs, native, samples, capfd):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "8x4", [_launch(16, 8, 64)], "8x4 ssaa 2", ssaa=2)


@pytest.mark.parametrize("nc,nf,qualifies", [(8, 16, False), (62, 128, False), (32, 64, True), (96, 32, True)])
def test_sample_counts_same_bits(pairs, native, samples, capfd, nc, nf, qualifies):
    """Samples per ray that are no multiple of 32 have no wave tiling and so no cut; 32 and 96 have blocks of 8 and 24 tiles."""
    off, on = pairs()
    _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, nc)] if qualifies else [], f"32x8 {nc}+{nf}", nc=nc, nf=nf)


@pytest.mark.parametrize("dtype", ("bf16x3", "f16x2"))
def test_split_arithmetics_keep_the_f32_sampling_pass(pairs, native, samples, capfd, dtype):
    off, on = pairs()
    _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 64)], f"32x8 {dtype}", dtype=dtype)


@pytest.mark.parametrize("mode,launches", [("coarse_only", []), ("skip_empty", [_launch(32, 8, 64)]), ("skip_dead", []), ("certify_zero", [])])
def test_other_render_modes_same_bits(pairs, native, samples, capfd, mode, launches):
    """coarse_only composites the coarse densities, skip_dead and certify_zero have their own sampling launches: none of them is cut.  A
    skip_empty render's sampling launch feeds the resampler alone and is."""
    off, on = pairs()
    plain, _ = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 64)], "32x8 plain")
    out, _ = _window(native, samples, capfd, off, on, "32x8", launches, f"32x8 {mode}", nf=0 if mode == "coarse_only" else 128, **{mode: True})
    if mode != "coarse_only":
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
def _skipped(sigma, t, far, w, h, threshold):
    """tiles the walk leaves out on an h x w window (rays row-major) when a ray counts as cut behind the first sample with T < threshold; T walks in float32"""
    nc = t.shape[1]
    delta = np.maximum(np.concatenate([t[:, 1:], np.full((len(t), 1), far, np.float32)], axis=1) - t, np.float32(0))
    alpha = np.float32(1) - np.exp(-sigma * delta, dtype=np.float32)
    T = np.ones(len(t), np.float32)
    first_behind = np.full(len(t), nc)                                          # index of the first sample behind the ray's cut
    for i in range(nc):
        live = first_behind == nc
        T = np.where(live, T * (np.float32(1) - alpha[:, i]), T).astype(np.float32)
        first_behind[live & (T < np.float32(threshold))] = i + 1
    last = first_behind.reshape(h // 4, 4, w // 8, 8).max(axis=(1, 3))          # behind it all 32 rays of a block are cut
    return int((nc // 4 - -(-last // 4)).sum())


def test_tiles_skipped_lies_in_the_host_bracket(pairs, native, samples, capfd):
    off, on = pairs()
    x0, y0, w, h = FIRST
    _, cuts = _window(native, samples, capfd, off, on, "32x8", [_launch(32, 8, 64)])
    cam = native.camera_from_samples(samples, 800, 800, 64)
    re_ = restate(GpuBackend(native, on.r), cam, 64, 128, FIRST, 0)
    sigma, t = np.asarray(re_["sigma_coarse"], np.float32), np.asarray(re_["t_coarse"], np.float32)
    far = np.float32(cam.far)
    lo = _skipped(sigma, t, far, w, h, 1e-4 * (1 - 1e-3))                      # a ray that comes that close is not cut there ...
    hi = _skipped(sigma, t, far, w, h, 1e-4 * (1 + 1e-3))                      # ... or is
    capfd.readouterr()
    with capfd.disabled():
        print(f"\ncoarsecut-count {FIRST}: tiles skipped {cuts[0][0]} of {cuts[0][1]} in {cuts[0][2]} blocks, host bracket [{lo}, {hi}]")
    assert lo <= cuts[0][0] <= hi and cuts[0][0] > 0, (cuts, lo, hi)


# ---- 3. synthetic networks ----------------------------------------------------------------------------------------------------------------
def _load_tensors(native, r, alpha_bias):
    """all weights and biases zero but the alpha head's bias, as both networks, through nerf_load_network_tensors"""
    f32p = C.POINTER(C.c_float)
    names, dims, arrs = [], [], []
    for name, k, n in SHAPES:
        names += [f"{name}_kernel", f"{name}_bias"]
        dims += [k, n, n, 0]
        arrs += [np.zeros(k * n, np.float32), np.full(n, alpha_bias if name == "alpha" else 0.0, np.float32)]
    c_names = (C.c_char_p * len(names))(*[s.encode() for s in names])
    c_dims = (C.c_int64 * len(dims))(*dims)
    c_data = (f32p * len(arrs))(*[a.ctypes.data_as(f32p) for a in arrs])
    for which in (0, 1):
        assert r._L.nerf_load_network_tensors(r.handle, which, len(names), c_names, c_dims, c_data) == 0, r._L.nerf_last_error(r.handle)
    r.coarse, r.fine = native.Network(r, 0), native.Network(r, 1)


@pytest.mark.parametrize("alpha_bias,every_block", [(1e4, True), (0.0, False)])
def test_fog_cuts_every_block_behind_its_first_tile_and_nothing_cuts_nothing(pairs, native, samples, capfd, alpha_bias, every_block):
    off, on = pairs(load=False)
    for c in (off, on):
        _load_tensors(native, c.r, alpha_bias)
    for window, (w, h) in (("32x8", (32, 8)), ("32x10", (32, 10))):
        tiles, blocks = _launch(w, h, 64)
        out, cuts = _window(native, samples, capfd, off, on, window, [(tiles, blocks)], f"{window} alpha bias {alpha_bias}")
        assert cuts[0][0] == (blocks * (64 // 4 - 1) if every_block else 0), cuts
        assert (out[2] >= 0.999).all() if every_block else (out[2] == 0.0).all()  # opaque fog / nothing at all


# ---- 4. the k-step diagnostic runs without the cut ----------------------------------------------------------------------------------------
def test_zskip_context_counts_every_sample(pairs, native, samples, capfd):
    zs_off, zs_on = pairs(zskip=True)
    off, on = pairs()
    render = lambda r: _render(native, samples, r, FIRST)
    a, c_on, g_on = zs_on.run(capfd, render)
    b, c_off, g_off = zs_off.run(capfd, render)
    assert c_on == [] and c_off == [], (c_on, c_off)
    assert g_on and g_on == g_off, (g_on, g_off)
    assert [t for n, _, t in g_on if n == SIGMA_RAYS] == [Z.n_waves(32 * 8 * 64) * 7 * 128], g_on     # seven ReLU layers of every wave of every sample
    plain, _ = _same(capfd, off, on, render, "32x8 plain", [_launch(32, 8, 64)])
    for k in range(3):
        _eq(a[k], plain[k], f"k-step diagnostic on / default, output {k}")
        _eq(b[k], plain[k], f"k-step diagnostic on, switched off / default, output {k}")


# ---- 5. the default asks for 16 blocks per workgroup ----------------------------------------------------------------------------------------
def test_default_context_cuts_large_launches_only(pairs, native, samples, capfd):
    off, _ = pairs()
    ctx = _Ctx(native, None)
    try:
        ctx.r.load_scene(SCENE)
        n_cus = ctx.r.device_info()["n_cus"]
        _window(native, samples, capfd, off, ctx, "32x8", [], "32x8 default context")          # 8 blocks: static walk
        rows = 4 * -(-16 * n_cus // 100)                                                       # 100 blocks per block row of the 800-pixel view
        below = (0, 300, 800, rows - 4)
        out, _ = _same(capfd, off, ctx, lambda r: _render(native, samples, r, below), "one block row short of 16 blocks per workgroup", [])
        crop = (0, 300, 800, rows)
        out, cuts = _same(capfd, off, ctx, lambda r: _render(native, samples, r, crop), "16 blocks per workgroup", [_launch(800, rows, 64)])
        assert cuts[0][0] > 0 and (out[2] > 0.99).any() and (out[2] < 0.01).any(), cuts
    finally:
        ctx.r.close()
