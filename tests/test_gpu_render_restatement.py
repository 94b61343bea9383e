"""The fused render path against its own restatement from the public stage calls (-m gpu).

Every kernel is held to the oracle when it is called on its own; the render path (ray-mode MLP launches, certify_zero's list mode,
the ray-sequential trunk with its colour passes, the split-arithmetic colour kernels, pass offsets, SSAA sub-rays) was seen only through
composited pixels, and a sample evaluated at the right position with ANOTHER ray's view direction moves a lego pixel by about 1e-6:
neither Gate 1 nor bit-identity between fused modes (which share ray = idx / samples_per_ray) can see it.  Here

  a. render_image == tests/helpers/render_restatement.restate(GpuBackend, ...) BIT FOR BIT: ray mode forms p = o + d * t with the
     multiply and the add rounded separately and then runs the per-column arithmetic of points mode, so the restatement (host points
     rounded the same way, Network.forward_batch with the ray's direction repeated per sample, stage_resample, stage_integrate) must
     carry the render's own bits -- in every arithmetic, with skip_empty / skip_dead / certify_zero, at sample counts that straddle the
     32-, 128- and 256-point tiles, ragged windows with a non-zero origin, SSAA 2 and 3, and passes that end inside the window;
  b. the probe frame (a fog whose colour follows direction strongly: one misrouted sample per ray moves half the pixels beyond 5e-4,
     tests/test_render_restatement_cpu.py) against the ORACLE evaluated on the render's own sample positions, at the unrelaxed Gate 1;
  c. the probe frame through render_image_multi (three contexts, contiguous and striped bands): band assembly re-bases ray indices too.
A MUTANT restatement (sample 0 of every ray given the previous ray's direction) must fail both a and b: the assertions bite.

hybrid_sampling is approximate by contract and stays out.

Measured on an MI355X: every equality below held at the first run -- f32, bf16x3, f16x2 and bf16, fused and with every exact mode, on
every window, shape, SSAA factor and pass size; no mode needed the Gate 1 fallback.  Probe frame against the oracle on the render's
samples: f32 max 4.8e-7 mean 6.6e-8, bf16x3 max 4.8e-7 mean 7.1e-8, f16x2 max 4.2e-7 mean 6.0e-8 (skip_dead: the same bits); bf16 against
the bf16 emulation max 1.9e-4 mean 3.2e-6, 97.1 dB; the mutant restatement max 2.9e-2 mean 9.1e-4, 53 % of the pixels above 5e-4.
The whole file runs in about 3 s."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import SCENE, psnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import render_restatement as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16x3", "f16x2", "bf16")
# what the API allows next to each arithmetic (nerf_render.cpp check_image_modes: certify_zero needs F32, BF16X3 or F16X2)
MODES = {"f32": ("skip_empty", "skip_dead", "certify_zero"), "bf16x3": ("skip_empty", "skip_dead", "certify_zero"),
         "f16x2": ("skip_empty", "skip_dead", "certify_zero"), "bf16": ("skip_empty", "skip_dead")}
# (n_coarse, n_fine, coarse_only): samples per ray 8, 2, 70, 33, 192, 300, 64, 20 -- rays that end inside a 32-sample wave tile and
# inside a 128- / 256-point workgroup tile, a ray longer than a tile, and the reference's branches without resampling
SHAPES = [(3, 5, False), (2, 5, False), (20, 50, False), (33, 0, False), (64, 128, False), (100, 200, False), (64, 0, True), (20, 0, True)]
# ray counts that are multiples of nothing, non-zero origins.  The first two see the model's silhouette at low sample counts and
# its body at high ones, the 96 x 96 window the other way round: together they hold white and non-white pixels at every shape
LEGO_WINDOWS = [(800, (311, 287, 13, 9)), (256, (121, 100, 7, 5)), (96, (19, 55, 7, 5))]
LEGO_SEED = 2 ** 40 + 7


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _diff(img, ref):
    """'' if img carries ref's bits, else a description of the difference."""
    if img.shape != ref.shape:
        return f"shape {img.shape} != {ref.shape}"
    bad = (_bits(img) != _bits(ref)).any(axis=-1)
    if not bad.any():
        return ""
    d = np.abs(img.astype(np.float64) - ref)
    return f"{int(bad.sum())} of {bad.size} pixels differ, max {d.max():.3e} mean {d.mean():.3e}, first at {tuple(np.argwhere(bad)[0])}"


def _gate1(img, ref):
    d = np.abs(img - ref)
    return d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(img, ref) >= 90.0


def _render(native, r, cam, nf, seed, crop, dtype, coarse_only=False, ssaa=1, **mode):
    return native.render_image(r.coarse, r.fine, cam, nf, seed=seed, crop=crop, coarse_only=coarse_only, ssaa=ssaa, dtype=dtype, **mode)


def _check_all_modes(native, r, cam, nf, seed, crop, dtype, want, what, coarse_only=False, ssaa=1):
    """The fused frame and every exact mode the API allows in this arithmetic against `want`; -> the list of differences."""
    out = []
    for mode in (None,) + MODES[dtype]:
        img = _render(native, r, cam, nf, seed, crop, dtype, coarse_only, ssaa, **({mode: True} if mode else {}))
        d = _diff(img, want)
        if d:
            out.append(f"{what} {dtype} {mode or 'fused'}: {d}")
    return out


# ---- a. lego ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nc,nf,coarse_only", SHAPES, ids=[f"{a}+{b}" if not c else f"coarse-only {a}" for a, b, c in SHAPES])
def test_lego_render_is_its_restatement(native, renderer, samples, nc, nf, coarse_only, dtype):
    be = RR.GpuBackend(native, renderer)
    failures, white = [], []
    for W, crop in LEGO_WINDOWS:
        cam = native.camera_from_samples(samples, W, W, nc)
        rs = RR.restate(be, cam, nc, nf, crop, LEGO_SEED, coarse_only=coarse_only, dtype=dtype)
        assert np.isfinite(rs["image"]).all()
        white.append((rs["image"] == 1.0).all(axis=2).reshape(-1))
        failures += _check_all_modes(native, renderer, cam, nf, LEGO_SEED, crop, dtype, rs["image"], f"{W}^2 {crop} {nc}+{nf}", coarse_only)
    white = np.concatenate(white)
    assert white.any() and not white.all()          # empty rays and rays through the model, both
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ssaa", [2, 3])
def test_lego_ssaa_render_is_its_restatement(native, renderer, samples, ssaa, dtype):
    """4 x 3 pixels = 8 x 6 / 12 x 9 sub-rays of the 2 x / 3 x camera, box-filtered: row-major sum, then one multiply by 1 / S^2."""
    cam = native.camera_from_samples(samples, 96, 96, 20)
    crop = (22, 56, 4, 3)
    rs = RR.restate(RR.GpuBackend(native, renderer), cam, 20, 50, crop, LEGO_SEED, ssaa=ssaa, dtype=dtype)
    assert rs["t_fine"].shape == (12 * ssaa * ssaa, 70)
    sub_white = (rs["image"] == 1.0).all(axis=2)
    assert sub_white.any() and not sub_white.all()
    failures = _check_all_modes(native, renderer, cam, 50, LEGO_SEED, crop, dtype, rs["image"], f"ssaa {ssaa}", ssaa=ssaa)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cap", [13, 50])
def test_lego_passes_that_end_inside_the_window(native, renderer, samples, monkeypatch, cap):
    """NERF_MAX_RAYS_PER_PASS (read when a context is created) = the window's width (one row per pass) and 50 (three rows per pass):
    a pass re-bases its ray index; the restatement knows nothing of passes."""
    W, crop = LEGO_WINDOWS[0]
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(cap))
    failures = []
    with native.Renderer(0) as r2:
        r2.load_scene(SCENE)
        for nc, nf in ((20, 50), (64, 128)):
            cam = native.camera_from_samples(samples, W, W, nc)
            for dtype in DTYPES:
                rs = RR.restate(RR.GpuBackend(native, renderer), cam, nc, nf, crop, LEGO_SEED, dtype=dtype)
                _, st = native.render_image(r2.coarse, r2.fine, cam, nf, seed=LEGO_SEED, crop=crop, dtype=dtype, return_stats=True)
                assert st.n_passes == -(-crop[3] // (cap // crop[2]))
                failures += _check_all_modes(native, r2, cam, nf, LEGO_SEED, crop, dtype, rs["image"], f"cap {cap} {nc}+{nf}")
    assert not failures, "\n".join(failures)


# ---- the probe ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(native, oracle, samples, tmp_path_factory):
    P = RR.PROBE
    root = RR.probe_scene(tmp_path_factory.mktemp("probe") / "scene")
    r = native.Renderer(0)
    r.load_scene(str(root))
    n = P["size"]
    p = types.SimpleNamespace(root=str(root), r=r, be=RR.GpuBackend(native, r), cam=native.camera_from_samples(samples, n, n, P["nc"]),
                              ocam=oracle.camera_from_samples(samples, n, n), nc=P["nc"], nf=P["nf"], seed=P["seed"], crop=(0, 0, n, n),
                              onets=(oracle.Net(str(root / "coarse")), oracle.Net(str(root / "fine"))), cache={})

    def restated(dtype, mutant=False):
        key = (dtype, mutant)
        if key not in p.cache:
            rs = RR.restate(p.be, p.cam, p.nc, p.nf, p.crop, p.seed, dtype=dtype, fine_dirs=RR.roll_first_sample if mutant else None)
            for a in rs.values():
                a.setflags(write=False)
            p.cache[key] = rs
        return p.cache[key]

    p.restated = restated
    yield p
    r.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_probe_render_is_its_restatement_and_not_the_mutant(native, probe, dtype):
    rs, mutant = probe.restated(dtype), probe.restated(dtype, mutant=True)
    for k in ("t_coarse", "sigma_coarse", "t_fine", "sigma_fine", "w_fine"):          # the mutant differs in colours alone
        assert np.array_equal(_bits(rs[k]), _bits(mutant[k])), k
    assert (rs["w_fine"][:, 0] > 0).mean() > 0.5      # the misrouted sample carries weight on 2 rays of 3 (the oracle: 0.667; ReLU zeros elsewhere)
    failures = _check_all_modes(native, probe.r, probe.cam, probe.nf, probe.seed, probe.crop, dtype, rs["image"], "probe")
    assert not failures, "\n".join(failures)
    img = _render(native, probe.r, probe.cam, probe.nf, probe.seed, None, dtype)       # the whole frame without a crop window
    assert not _diff(img, rs["image"])
    assert not np.array_equal(_bits(img), _bits(mutant["image"]))                      # ONE wrong direction per ray: the equality fails
    assert (_bits(img) != _bits(mutant["image"])).any(axis=2).mean() > 0.5             # ... on every such pixel (the oracle: 0.667)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ssaa", [2, 3])
def test_probe_ssaa_render_is_its_restatement(native, probe, ssaa, dtype):
    crop = (5, 4, 4, 3)
    rs = RR.restate(probe.be, probe.cam, probe.nc, probe.nf, crop, probe.seed, ssaa=ssaa, dtype=dtype)
    failures = _check_all_modes(native, probe.r, probe.cam, probe.nf, probe.seed, crop, dtype, rs["image"], f"probe ssaa {ssaa}", ssaa=ssaa)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cap", [12, 50])
def test_probe_passes_that_end_inside_the_frame(native, probe, monkeypatch, cap):
    monkeypatch.setenv("NERF_MAX_RAYS_PER_PASS", str(cap))
    failures = []
    with native.Renderer(0) as r2:
        r2.load_scene(probe.root)
        for dtype in DTYPES:
            _, st = native.render_image(r2.coarse, r2.fine, probe.cam, probe.nf, seed=probe.seed, dtype=dtype, return_stats=True)
            assert st.n_passes == -(-12 // (cap // 12))
            failures += _check_all_modes(native, r2, probe.cam, probe.nf, probe.seed, probe.crop, dtype, probe.restated(dtype)["image"], f"cap {cap}")
    assert not failures, "\n".join(failures)


# ---- b. the probe against the oracle on the render's own samples --------------------------------------------------------------------
def _oracle_on_render_samples(oracle, probe, rs, bf16=False):
    """oracle fine network at the restatement's float32 points with each ray's direction, composited by oracle.integrate_ray."""
    R, n = rs["t_fine"].shape
    net = probe.onets[1]
    rgb, sg = (net.forward_batch_bf16 if bf16 else net.forward_batch)(rs["pts_fine"], np.repeat(rs["dirs"], n, axis=0))
    rgb, sg, far = rgb.reshape(R, n, 3), sg.reshape(R, n), float(probe.ocam.far)
    return np.stack([oracle.integrate_ray(rgb[r], sg[r], rs["t_fine"][r], far) for r in range(R)]).reshape(rs["image"].shape)


def test_probe_coarse_samples_are_the_oracles(oracle, probe):
    rs = probe.restated("f32")
    near, far = float(probe.ocam.near), float(probe.ocam.far)
    for r in range(144):
        assert np.array_equal(_bits(rs["t_coarse"][r]), _bits(oracle.stratified_samples(probe.seed, r, near, far, probe.nc))), r
        i, j = divmod(r, 12)
        assert np.array_equal(_bits(rs["dirs"][r]), _bits(oracle.normalize(oracle.get_ray_dir(probe.ocam, i, j)))), r


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16x2"])
def test_probe_frame_against_the_oracle_on_its_own_samples(native, oracle, probe, dtype):
    """Both sides use the render's sample positions: no fine sample can be relocated, so the outliers _fog_gate
    (tests/test_gpu_hybrid_validation.py) exists for cannot occur and Gate 1 holds unrelaxed (max <= 5e-4, mean <= 1e-5, PSNR >= 90 dB).
    Measured (fused = skip_dead, bit for bit): f32 max 4.77e-7 mean 6.62e-8 (140.0 dB), bf16x3 max 4.77e-7 mean 7.12e-8 (139.4 dB),
    f16x2 max 4.17e-7 mean 5.97e-8 (141.1 dB); the mutant restatement: max 2.91e-2, mean 9.05e-4, 53 % of the pixels above 5e-4."""
    rs = probe.restated(dtype)
    ref = _oracle_on_render_samples(oracle, probe, rs)
    for mode in ({}, dict(skip_dead=True)):
        img = _render(native, probe.r, probe.cam, probe.nf, probe.seed, None, dtype, **mode)
        d = np.abs(img - ref)
        print(f"\nprobe {dtype} {mode or 'fused'} vs oracle on the render's samples: max {d.max():.3e} mean {d.mean():.3e} psnr {psnr(img, ref):.1f} dB")
        assert _gate1(img, ref), (dtype, mode, d.max(), d.mean(), psnr(img, ref))
    mutant = probe.restated(dtype, mutant=True)["image"]
    d = np.abs(mutant - ref)
    print(f"mutant restatement vs the same reference: max {d.max():.3e} mean {d.mean():.3e}, {(d.max(axis=2) > 5e-4).mean():.2f} of the pixels above 5e-4")
    assert not _gate1(mutant, ref)                                                      # one wrong direction per ray: Gate 1 fails


def test_probe_bf16_frame_against_the_bf16_emulation(native, oracle, probe):
    """bf16 is its own arithmetic: its checker is the oracle's bf16-operand emulation at PSNR >= 30 dB, as in tests/test_gpu_bf16*.py."""
    rs = probe.restated("bf16")
    ref = _oracle_on_render_samples(oracle, probe, rs, bf16=True)
    for mode in ({}, dict(skip_dead=True)):
        img = _render(native, probe.r, probe.cam, probe.nf, probe.seed, None, "bf16", **mode)
        d = np.abs(img - ref)
        print(f"\nprobe bf16 {mode or 'fused'} vs the bf16 emulation on the render's samples: max {d.max():.3e} mean {d.mean():.3e} psnr {psnr(img, ref):.1f} dB")
        assert psnr(img, ref) >= 30.0


# ---- c. row order -------------------------------------------------------------------------------------------------------------------
def test_probe_multi_context_bands_keep_the_row_order(native, probe):
    """Three contexts on device 0, gather = host: contiguous bands (a plain render) and bands striped row by row (skip_dead: nerf_multi.cpp
    deals rows out round-robin when cost follows the scene).  The frame is the single-context frame = the restatement, bit for bit."""
    rs = [native.Renderer(0) for _ in range(3)]
    try:
        for r in rs:
            r.load_scene(probe.root)
        want = probe.restated("f32")["image"]
        for kw in ({}, dict(skip_dead=True)):
            img = native.render_image_multi(rs, probe.cam, probe.nf, gather="host", seed=probe.seed, **kw)
            assert not _diff(img, want), kw
            assert np.array_equal(img, _render(native, probe.r, probe.cam, probe.nf, probe.seed, None, "f32", **kw))
        x3 = native.render_image_multi(rs, probe.cam, probe.nf, gather="host", seed=probe.seed, dtype="bf16x3", skip_dead=True)
        assert not _diff(x3, probe.restated("bf16x3")["image"])
    finally:
        for r in rs:
            r.close()
