"""Display-ready RGBA8 on the device (nerf_render_image_rgba8 and its device, multi and stage siblings): the bytes against a NumPy
float32 restatement of the contract in include/nerf_mi355x.h, against the float entry points + the host quantiser, and across the
device, multi-context and validation paths.

The contract, per ray: C = sum_i w_i c_i and A = sum_i w_i, sequential f32 sums with separate multiply and add; opaque = C + B * (1 - A)
(multiply and add rounded separately, alpha 255); premultiplied = C with alpha A; straight = C / A (IEEE f32 division) where A > 0 else
0, alpha A; every channel quantised as clamp(v, 0, 1) * 255 + 0.5 truncated, NaN -> 0."""
import ctypes as C

import numpy as np
import pytest

from conftest import SCENE
from helpers import sampling_cases as SC

pytestmark = pytest.mark.gpu

f32 = np.float32
MODES = ["opaque", "premultiplied", "straight"]
BACKGROUNDS = [None, (0.0, 0.0, 0.0), (0.25, 0.5, 0.75)]
STAGE_N = [1, 16, 17, 33, 192]   # k_composite stages 16 samples at a time


# ---- the contract in NumPy float32 ------------------------------------------------------------------------------------------------
def q8(v):
    """The reference's quantiser (save_ppm, src/lib.rs:573-577): every operation rounded to f32, NaN -> 0."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        c = np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)
        q = ((c * f32(255)).astype(f32) + f32(0.5)).astype(f32)
        return np.where(np.isnan(q), 0, np.nan_to_num(q)).astype(np.uint8)   # float -> u8 truncates; q lies in [0.5, 255.5]


def sums(w, c):
    """C (R, 3) and A (R,) from the weights (R, n) and colours (R, n, 3): sample order, f32, separate multiply and add."""
    R, n = w.shape
    acc = np.zeros(R, f32)
    col = np.zeros((R, 3), f32)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            col = (col + (c[:, i, :] * w[:, i, None]).astype(f32)).astype(f32)
            acc = (acc + w[:, i]).astype(f32)
    return col, acc


def pack(col, acc, background, mode):
    """(R, 4) bytes of the contract from the per-pixel C and A."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "opaque":
            b = np.ones(3, f32) if background is None else np.asarray(background, f32)
            rest = (f32(1) - acc).astype(f32)
            rgb = (col + (b[None, :] * rest[:, None]).astype(f32)).astype(f32)
            alpha = np.full(len(acc), 255, np.uint8)
        else:
            rgb = col                                                # C + 0 * (1 - A) = C
            if mode == "straight":
                some = acc > 0
                rgb = np.where(some[:, None], (col / np.where(some, acc, f32(1))[:, None]).astype(f32), f32(0)).astype(f32)
            alpha = q8(acc)
    return np.concatenate([q8(rgb), alpha[:, None]], axis=1)


def test_numpy_quantiser_is_the_host_quantiser(native):
    """A self-check of this file's reference, not of the feature: q8 above must be the host quantiser that existed before the RGBA8
    entry points did (so this one test also passes without them); every other test here calls a new symbol."""
    v = np.concatenate([np.linspace(-0.1, 1.1, 4099), [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], (np.arange(256) + 0.5) / 255]).astype(f32)
    v = np.resize(v, (len(v) // 3) * 3)
    assert np.array_equal(q8(v), native.quantize_rgb8(v.reshape(-1, 3)).reshape(-1))


# ---- 1. stage level, exact -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage_inputs(oracle):
    """Per n: the 130 rays of the "density" and "one_hot" families (ray r is the same ray whatever the number of rays asked for)."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = {fam: SC.FAMILIES[fam](oracle, max(SC.COMPOSITE_RAYS), n) for fam in ("density", "one_hot")}
        return cache[n]
    return get


def _check_batch(native, renderer, t, sigma, tag):
    """One batch of rays through stage_integrate (weights, float colour) and through every mode x background of stage_integrate_rgba8."""
    R, n = t.shape
    c = SC.distinct_colours(R, n)
    rgb_f, w = renderer.stage_integrate(c, sigma, t, SC.FAR)
    col, acc = sums(w, c)
    empty = acc == 0
    for mode in MODES:
        for bg in BACKGROUNDS:
            got = renderer.stage_integrate_rgba8(c, sigma, t, SC.FAR, background=bg, alpha=mode)
            assert got.shape == (R, 4) and got.dtype == np.uint8
            want = pack(col, acc, bg, mode)
            assert np.array_equal(got, want), (tag, mode, bg, np.argwhere(got != want)[:4])
            if mode == "opaque":                                      # A == 0: exactly the quantised background, alpha 255
                b = q8(np.ones(3, f32) if bg is None else np.asarray(bg, f32))
                assert (got[empty] == np.concatenate([b, [255]])).all(), (tag, mode, bg)
            else:                                                     # ... and exactly transparent black in the two alpha modes
                assert (got[empty] == 0).all(), (tag, mode, bg)
    # over white, opaque: the bytes of the float entry point + the host quantiser
    assert np.array_equal(renderer.stage_integrate_rgba8(c, sigma, t, SC.FAR), native.quantize_rgba8(rgb_f)), tag
    return acc


@pytest.mark.parametrize("n", STAGE_N)
@pytest.mark.parametrize("R", SC.COMPOSITE_RAYS)
def test_stage_bytes_equal_the_contract(native, renderer, stage_inputs, R, n):
    """A single ray cannot hold three kinds of opacity: for R = 1 the density family is launched three times as a one-ray batch, with the
    first ray of each kind among its 130 (so the launch shape is still one ray); for R >= 63 the batch is the family's first R rays."""
    fams = stage_inputs(n)
    accs = []
    for fam, (t, sigma) in fams.items():
        if R == 1 and fam == "density" and n >= 16:
            _, w = renderer.stage_integrate(SC.distinct_colours(*t.shape), sigma, t, SC.FAR)
            a_all = sums(w, np.zeros(t.shape + (3,), f32))[1]
            picks = [np.flatnonzero(m)[0] for m in (a_all == 0, (a_all > 0) & (a_all < 0.99), a_all >= 0.99)]
            for r in picks:
                accs.append(_check_batch(native, renderer, t[r:r + 1], sigma[r:r + 1], (fam, R, n, int(r))))
        else:
            accs.append(_check_batch(native, renderer, t[:R], sigma[:R], (fam, R, n)))
    acc = np.concatenate(accs)
    if n >= 16:   # the inputs hold empty rays, (nearly) opaque rays and rays in between: every branch of the pack sees data
        assert (acc == 0).any() and (acc >= 0.99).any() and ((acc > 0) & (acc < 0.99)).any(), (R, n)


def test_stage_nan_colour_gives_zero_in_that_channel(renderer, stage_inputs):
    R, n = 65, 17
    t, sigma = (a[:R] for a in stage_inputs(n)["density"])
    c = SC.distinct_colours(R, n)
    c[5, 3, 1] = np.nan
    _, w = renderer.stage_integrate(c, sigma, t, SC.FAR)
    col, acc = sums(w, c)
    assert np.isnan(col[5, 1]) and np.isfinite(np.delete(col, 5, axis=0)).all()
    for mode in MODES:
        for bg in BACKGROUNDS:
            got = renderer.stage_integrate_rgba8(c, sigma, t, SC.FAR, background=bg, alpha=mode)
            assert got[5, 1] == 0
            assert np.array_equal(got, pack(col, acc, bg, mode)), (mode, bg)


# ---- 2. frame level ---------------------------------------------------------------------------------------------------------------------
# 41 x 23 pixels of the 100 x 100 lego view at 16 + 32 samples: 943 rays (14 waves of k_composite and 47 rays of a 15th), neither side a
# multiple of 8.  Chosen with the CPU oracle's opacity map of that view: 376 pixels of opacity 0, 385 of opacity >= 0.99 and 126 between
# 0.05 and 0.95 (the silhouette).
WINDOW = (6, 44, 41, 23)
NF = 32
BG = (0.25, 0.5, 0.75)


@pytest.fixture(scope="module")
def cam100(native, samples):
    return native.camera_from_samples(samples, 100, 100, 16)


@pytest.fixture(scope="module")
def frame(native, renderer, cam100):
    rgb, _, opacity = native.render_image(renderer.coarse, renderer.fine, cam100, NF, seed=0, crop=WINDOW, aux=True)
    assert (opacity == 0).sum() > 50 and (opacity >= 0.99).sum() > 50 and ((opacity > 0.05) & (opacity < 0.95)).sum() > 20
    return rgb, opacity


def _rgba(native, r, cam, **kw):
    kw.setdefault("crop", WINDOW)
    return native.render_image_rgba8(r.coarse, r.fine, cam, NF, seed=0, **kw)


def _steps(a, b):
    return np.abs(a.astype(np.int32) - b.astype(np.int32)).max()


FRAME_MODES = {"f32": {}, "skip_dead": dict(skip_dead=True), "certify_zero": dict(certify_zero=True), "f16x2": dict(dtype="f16x2"),
               "ssaa2": dict(ssaa=2), "band": dict(band=(1, 3, 1))}


@pytest.mark.parametrize("mode", list(FRAME_MODES))
def test_opaque_over_white_is_the_quantised_float_frame(native, renderer, cam100, frame, mode):
    kw = FRAME_MODES[mode]
    want = native.render_image(renderer.coarse, renderer.fine, cam100, NF, seed=0, crop=WINDOW, **kw)
    got = _rgba(native, renderer, cam100, **kw)
    assert got.shape == want.shape[:2] + (4,) and got.dtype == np.uint8
    assert np.array_equal(got, native.quantize_rgba8(want))
    assert np.array_equal(got, _rgba(native, renderer, cam100, background=(1.0, 1.0, 1.0), **kw))   # B = 1 is NULL


@pytest.mark.parametrize("ssaa", [1, 2])
def test_premultiplied_and_straight_frames(native, renderer, cam100, frame, ssaa):
    kw = dict(ssaa=ssaa)
    rgb, _, opacity = native.render_image(renderer.coarse, renderer.fine, cam100, NF, seed=0, crop=WINDOW, aux=True, **kw)
    pre = _rgba(native, renderer, cam100, alpha="premultiplied", background=BG, **kw)     # the background is ignored
    black = _rgba(native, renderer, cam100, background=(0.0, 0.0, 0.0), **kw)
    straight = _rgba(native, renderer, cam100, alpha="straight", **kw)
    assert np.array_equal(pre[..., 3], q8(opacity)) and np.array_equal(straight[..., 3], q8(opacity))
    assert np.array_equal(pre[..., :3], black[..., :3]) and (black[..., 3] == 255).all()
    fg = (rgb - (f32(1) - opacity)[..., None]).astype(f32)          # the float detour: the foreground rebuilt from the frame over white
    d_pre = _steps(pre[..., :3], q8(fg))
    some = opacity > 0
    assert (straight[~some] == 0).all() and (pre[~some] == 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = q8(np.clip(fg[some] / opacity[some][:, None], 0, 1))
    d_str = _steps(straight[..., :3][some], want)
    print(f"ssaa {ssaa}: premultiplied within {d_pre} step(s) of the float detour, straight within {d_str}; smallest opacity > 0: {opacity[some].min():.3e}")
    assert d_pre <= 1
    assert d_str <= 1


def test_opaque_over_a_colour(native, renderer, cam100, frame):
    rgb, opacity = frame
    got = _rgba(native, renderer, cam100, background=BG)
    assert (got[..., 3] == 255).all()
    assert (got[opacity == 0][:, :3] == q8(np.asarray(BG, f32))).all()
    rest = (f32(1) - opacity)[..., None]
    rebuilt = (rgb - rest) + np.asarray(BG, f32) * rest
    d = _steps(got[..., :3], q8(rebuilt.astype(f32)))
    print(f"opaque over {BG}: within {d} step(s) of the value rebuilt from the float maps")
    assert d <= 1


# ---- 3. device variant ------------------------------------------------------------------------------------------------------------------
def test_device_variant_on_a_stream_of_its_own(native, renderer, cam100):
    import torch
    stream = torch.cuda.Stream()
    for kw in (dict(alpha="straight"), dict(background=BG, ssaa=2)):
        host = _rgba(native, renderer, cam100, **kw)
        out = torch.full(host.shape, 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert native.render_image_rgba8(renderer.coarse, renderer.fine, cam100, NF, seed=0, crop=WINDOW, device_out=out.data_ptr(),
                                         stream=stream.cuda_stream, **kw) is None
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), host), kw


# ---- 4. multi ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(native):
    rs = [native.Renderer(0) for _ in range(3)]
    for r in rs:
        r.load_scene(SCENE)
    yield rs
    for r in rs:
        r.close()


@pytest.mark.parametrize("striped", [False, True], ids=["contiguous", "striped"])
@pytest.mark.parametrize("gather", ["host", "peer", "rccl"])
def test_multi_is_byte_identical_to_one_context(native, renderer, cam100, three, gather, striped):
    kw = dict(seed=0, crop=(3, 40, 43, 31), skip_dead=striped)      # 31 rows: ragged over three bands; 43 columns: odd band sizes
    for extra in (dict(), dict(alpha="straight"), dict(background=BG)):
        ref = native.render_image_rgba8(renderer.coarse, renderer.fine, cam100, NF, **kw, **extra)
        got = native.render_image_multi_rgba8(three, cam100, NF, gather=gather, **kw, **extra)
        assert np.array_equal(got, ref), extra
        assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 50          # a picture, not a constant


# ---- 5. validation ------------------------------------------------------------------------------------------------------------------------
def test_validation_leaves_the_context_usable(native, renderer, cam100, frame):
    from nerf_rs_amd import _lib
    L = native.load_library()
    opts = native.RenderOpts(16, NF, crop=WINDOW).to_c()
    good = _rgba(native, renderer, cam100)
    out = np.empty_like(good)

    def call(bg, mode, ptr):
        b = None if bg is None else np.asarray(bg, f32)
        rc = L.nerf_render_image_rgba8(renderer.handle, C.byref(cam100.c), C.byref(opts), None if b is None else b.ctypes.data_as(_lib.f32p),
                                       mode, ptr, None)
        return rc, (L.nerf_last_error(renderer.handle) or b"").decode()
    p = out.ctypes.data_as(_lib.u8p)
    for bg, mode, ptr, word in ((None, 3, p, "alpha_mode"), (None, -1, p, "alpha_mode"), ((0.5, np.nan, 0.5), 0, p, "background"),
                                ((np.inf, 0.0, 0.0), 0, p, "background"), (None, 0, None, "NULL")):
        rc, msg = call(bg, mode, ptr)
        assert rc == -1 and word in msg, (bg, mode, rc, msg)
        assert np.array_equal(_rgba(native, renderer, cam100), good)
    rc, _ = call((-3.0, 0.5, 7.0), 0, p)          # finite values outside [0, 1] are allowed: the quantiser clamps
    assert rc == 0 and (out[frame[1] == 0][:, :3] == (0, 128, 255)).all()
    with pytest.raises(native.NerfError):
        native.render_image_rgba8(renderer.coarse, renderer.fine, cam100, NF, crop=WINDOW, alpha="additive")
    with pytest.raises(native.NerfError):
        renderer.stage_integrate_rgba8(np.zeros((1, 1, 3)), np.zeros((1, 1)), np.full((1, 1), 3.0), 6.0, alpha=7)


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_library_frame_as_pam(native, renderer, cam100, tmp_path):
    import os
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "nerf-rs_amd", "nerf_cli")
    base = [exe, "--scene", SCENE, "--width", "100", "--height", "100", "--coarse", "16", "--fine", str(NF), "--out", str(tmp_path / "a.ppm")]
    for k, extra in enumerate((["--alpha", "straight"], ["--background", "0.25,0.5,0.75", "--devices", "0,0", "--gather", "peer"])):
        pam = tmp_path / f"f{k}.pam"
        res = subprocess.run(base + ["--rgba", str(pam)] + extra, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        want = native.render_image_rgba8(renderer.coarse, renderer.fine, cam100, NF, seed=0,
                                         **(dict(alpha="straight") if k == 0 else dict(background=BG)))
        head = b"P7\nWIDTH 100\nHEIGHT 100\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n"
        assert pam.read_bytes() == head + want.tobytes()
    assert subprocess.run(base + ["--rgba", str(tmp_path / "x.pam"), "--alpha", "additive"], capture_output=True).returncode == 2
