"""The sampling and compositing kernels (sampling_kernels.hip: k_ray_dirs, k_stratified, k_resample, k_composite, k_box_downsample)
against the CPU oracle AWAY from the shipped 64 + 128 shape (-m gpu): every width of the register sort and of the LDS sort, more than 64
coarse samples (second trips of the 64-lane loops), draws on bin edges and outside [0, 1), zero-width bins, both halves of the 64-bit
seed, pixel indices up to 2^32 - 1, 1 to 130 rays through k_composite's 64-ray staging, 1 to 1070 samples per ray, SSAA 3.

Tolerances (no others are used here):
  w    <= 2e-6 abs against oracle.compute_weights  (expf ulps only; the project's stated tolerance, tests/test_gpu_parity.py)
  rgb  <= 5e-6 abs against oracle.integrate_ray
  Gate 1 for rendered pixels (max <= 5e-4, mean <= 1e-5, PSNR >= 90 dB)
  everything else BIT-EQUAL: the kernels are built without contraction and with correctly rounded division, so from the weights on both
  sides do the same IEEE operations in the same order.  The oracle is therefore fed the GPU's own w: that removes the one legitimate
  difference (expf) from the CDF, the draws and the sort, and no tolerance is needed there.
Near-cut rays (tests/helpers/sampling_cases.py: transmittance within a relative 1e-3 of the 1e-4 cut, where an ulp of expf may move
the cut by one sample) are left out of the w / rgb comparisons; tests/test_sampling_cases_cpu.py caps them at 2 % of a family.  On
one-hot rays (alpha exactly 0 or 1) w and rgb are bit-equal as well."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import psnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sampling_cases as S

pytestmark = pytest.mark.gpu

W_TOL, RGB_TOL = 2e-6, 5e-6
FAR = S.FAR


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- k_resample ---------------------------------------------------------------------------------------------------------------------
def _check_downstream(oracle, out, t, u, nf, what):
    """cdf, draws and merged samples of one stage_resample call, bit for bit, from the GPU's own weights on."""
    for r in range(len(t)):
        tn, cdf = oracle.sample_importance_u(u[r], t[r], out["w"][r])
        assert _same_bits(out["cdf"][r], cdf), (what, r, "cdf")
        assert _same_bits(out["t_new"][r], tn), (what, r, "t_new", np.flatnonzero(_bits(out["t_new"][r]) != _bits(tn))[:8])
        merged = np.concatenate([t[r], tn])
        assert _same_bits(out["t_fine"][r], oracle.sort_ascending(merged)), (what, r, "t_fine")
        assert np.array_equal(out["t_fine"][r], np.sort(merged)), (what, r, "t_fine vs np.sort")   # a second, unrelated sort


def _check_resample(renderer, oracle, family, t, s, nf):
    R, nc = t.shape
    w_ref = np.stack([oracle.compute_weights(s[r], t[r], FAR) for r in range(R)])
    keep = np.ones(R, bool) if family == "one_hot" else ~S.near_cut_mask(s, t)
    out = None
    for k, seed in enumerate(S.SEEDS):    # the in-kernel Philox stream: key = both halves of the seed, counter = (pixel, 1, draw / 4, 0)
        pix = np.array([S.PIXELS[(r + k) % len(S.PIXELS)] for r in range(R)], np.uint32)
        out = renderer.stage_resample(t, s, nf, FAR, seed=seed, pixel_index=pix)
        d = np.abs(out["w"] - w_ref)[keep]
        print(f"{family} {nc}+{nf} seed {seed}: max |dw| = {d.max() if d.size else 0.0:.2e} over {int(keep.sum())} of {R} rays")
        assert d.size == 0 or d.max() <= W_TOL
        if family == "one_hot":
            assert _same_bits(out["w"], w_ref)
        u = np.array([[oracle.uniform(seed, int(pix[r]), 1, j) for j in range(nf)] for r in range(R)], np.float32)
        _check_downstream(oracle, out, t, u, nf, (family, nc, nf, seed))
        for r in range(R):
            assert _same_bits(out["t_new"][r], oracle.sample_importance(seed, int(pix[r]), t[r], out["w"][r], nf)), (family, seed, r)
    # explicit uniforms, built from the GPU's own CDF (just shown to be the oracle's CDF of the GPU's weights): draws ON its bin edges
    u = np.stack([S.explicit_uniforms(out["cdf"][r], nf, r) for r in range(R)])
    out_u = renderer.stage_resample(t, s, nf, FAR, u=u)
    assert _same_bits(out_u["w"], out["w"]) and _same_bits(out_u["cdf"], out["cdf"])
    _check_downstream(oracle, out_u, t, u, nf, (family, nc, nf, "explicit u"))


@pytest.mark.parametrize("family", list(S.FAMILIES))
@pytest.mark.parametrize("nc,nf", S.RESAMPLE_SHAPES)
def test_resample_vs_oracle(renderer, oracle, nc, nf, family):
    t, s = S.FAMILIES[family](oracle, S.RESAMPLE_RAYS, nc)
    _check_resample(renderer, oracle, family, t, s, nf)


@pytest.mark.parametrize("n_rays", [1, 4, 5])
def test_resample_ray_counts(renderer, oracle, n_rays):
    """A workgroup holds four rays: one ray, a full group, a full group and one more."""
    for family in S.FAMILIES:
        t, s = S.FAMILIES[family](oracle, n_rays, 65)
        _check_resample(renderer, oracle, family, t, s, 63)


@pytest.mark.parametrize("nc", S.WIDE_NC)
def test_resample_edge_draw_takes_the_first_matching_bin(renderer, oracle, nc):
    """A draw ON cdf[j] belongs to bin j (src/lib.rs:330-333: the first j with cdf[j] <= u < cdf[j+1]).  On evenly spaced samples the
    bin below gives the same float; on rays whose neighbouring t differ by more than a factor 2 it does not
    (sampling_cases.wide_ratio_rays).  Enough draws for every edge, the float below it and the values no bin matches."""
    t, s = S.wide_ratio_rays(S.RESAMPLE_RAYS, nc)
    _check_resample(renderer, oracle, "wide_ratio", t, s, 2 * (nc - 1) + 5)


# ---- k_stratified, k_ray_dirs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 2 ** 32 + 5, 2 ** 63 + 11])
def test_stratified_counts_and_seeds(renderer, native, oracle, samples, seed):
    cam = native.camera_from_samples(samples, 800, 800)
    near, far = float(samples["near"]), float(samples["far"])
    x0, y0, w, h = 100, 200, 7, 3
    for count in (1, 2, 3, 4, 5, 7, 8, 65, 257, 1000):   # a thread owns four samples: ragged last quads, several blocks
        t = renderer.stage_stratified(cam, x0, y0, w, h, count, seed=seed)
        for i in range(h):
            for j in range(w):
                assert _same_bits(t[i, j], oracle.stratified_samples(seed, (y0 + i) * 800 + x0 + j, near, far, count)), (count, i, j)


def test_far_corner_of_a_large_frame(renderer, native, oracle, samples):
    """A 10 x 5 window in the far corner of a 5000 x 3000 frame: pixel indices of about 1.5e7 (the shipped frame stops at 6.4e5)."""
    W, H = 5000, 3000
    cam, ocam = native.camera_from_samples(samples, W, H), oracle.camera_from_samples(samples, W, H)
    near, far = float(samples["near"]), float(samples["far"])
    x0, y0, w, h = W - 10, H - 5, 10, 5
    dirs = renderer.stage_ray_dirs(cam, x0, y0, w, h, normalize=True)
    raw = renderer.stage_ray_dirs(cam, x0, y0, w, h, normalize=False)
    for count, seed in ((5, 2 ** 32 + 5), (65, 2 ** 63 + 11)):
        t = renderer.stage_stratified(cam, x0, y0, w, h, count, seed=seed)
        for i in range(h):
            for j in range(w):
                assert _same_bits(t[i, j], oracle.stratified_samples(seed, (y0 + i) * W + x0 + j, near, far, count)), (count, i, j)
    for i in range(h):
        for j in range(w):
            d = oracle.get_ray_dir(ocam, y0 + i, x0 + j)
            assert _same_bits(raw[i, j], d) and _same_bits(dirs[i, j], oracle.normalize(d)), (i, j)


# ---- k_composite --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _composite_reference(oracle, family, n):
    """Inputs and oracle results of a family at the largest ray count, computed once: ray r is the same ray at every ray count."""
    R = max(S.COMPOSITE_RAYS)
    t, s = S.FAMILIES[family](oracle, R, n)
    col = np.random.default_rng([S.BASE_SEED, 5, n]).uniform(size=(R, n, 3)).astype(np.float32)
    w = np.stack([oracle.compute_weights(s[r], t[r], FAR) for r in range(R)])
    rgb = np.stack([oracle.integrate_ray(col[r], s[r], t[r], FAR) for r in range(R)])
    for a in (t, s, col, w, rgb):
        a.setflags(write=False)
    return t, s, col, w, rgb, ~S.near_cut_mask(s, t)


@pytest.mark.parametrize("n", S.COMPOSITE_N)
@pytest.mark.parametrize("n_rays", S.COMPOSITE_RAYS)
def test_composite_vs_oracle(renderer, oracle, n_rays, n):
    for family in ("density", "duplicate"):
        t, s, col, w_ref, rgb_ref, keep = (a[:n_rays] for a in _composite_reference(oracle, family, n))
        rgb, w = renderer.stage_integrate(col, s, t, FAR)
        dw, dc = np.abs(w - w_ref)[keep], np.abs(rgb - rgb_ref)[keep]
        print(f"{family} {n_rays} x {n}: max |dw| = {dw.max() if dw.size else 0.0:.2e}, max |drgb| = {dc.max() if dc.size else 0.0:.2e}, "
              f"{int(keep.sum())} of {n_rays} rays")
        assert dw.size == 0 or (dw.max() <= W_TOL and dc.max() <= RGB_TOL)
        assert np.isfinite(rgb).all() and np.isfinite(w).all()
    # one-hot rays with a distinct colour in every (ray, sample, channel): one element staged into the wrong slot is a wrong colour
    t, s, k = S.one_hot_rays(oracle, n_rays, n, offset=sum(r for r in S.COMPOSITE_RAYS if r < n_rays))
    col = S.distinct_colours(n_rays, n)
    rgb, w = renderer.stage_integrate(col, s, t, FAR)
    w_ref = np.stack([oracle.compute_weights(s[r], t[r], FAR) for r in range(n_rays)])
    rgb_ref = np.stack([oracle.integrate_ray(col[r], s[r], t[r], FAR) for r in range(n_rays)])
    assert _same_bits(w, w_ref), np.argwhere(_bits(w) != _bits(w_ref))[:8]
    assert _same_bits(rgb, rgb_ref), np.argwhere(_bits(rgb) != _bits(rgb_ref))[:8]
    hit = k < n
    assert np.array_equal(rgb[hit], col[np.flatnonzero(hit), k[hit]]) and np.all(rgb[~hit] == 1.0)


# ---- whole renders against the live oracle ------------------------------------------------------------------------------------------
def _gate1(img, ref):
    d = np.abs(img - ref)
    assert d.max() <= 5e-4 and d.mean() <= 1e-5 and psnr(img, ref) >= 90.0, (d.max(), d.mean(), psnr(img, ref))


@pytest.mark.parametrize("W,nc,nf,crop,seed,ssaa", [
    (256, 100, 200, (180, 135, 8, 6), 2 ** 40 + 7, 1),   # 300 samples: LDS sort of 512 with 212 pads, a partial last 32-sample chunk
    (256, 64, 256, (180, 135, 8, 6), 11, 1),             # 320 samples
    (96, 200, 824, (66, 54, 4, 3), 12, 1),               # 1024 samples: an LDS sort without padding
    (96, 64, 128, (19, 55, 6, 4), 13, 3),                # the shipped counts through a 3 x 3 box filter
])
def test_render_vs_live_oracle(renderer, native, oracle, oracle_nets, samples, W, nc, nf, crop, seed, ssaa):
    """Windows on the model's silhouette: the oracle's image holds pure-white (empty) and non-white pixels."""
    cam = native.camera_from_samples(samples, W, W, nc)
    ref = oracle.render_image(*oracle_nets, oracle.camera_from_samples(samples, W, W), oracle.make_opts(nc, nf, crop=crop, seed=seed, ssaa=ssaa))
    white = (ref == 1.0).all(axis=2)
    assert white.any() and not white.all()
    R = lambda **kw: native.render_image(renderer.coarse, renderer.fine, cam, nf, seed=seed, crop=crop, ssaa=ssaa, **kw)  # noqa: E731
    img = R()
    d = np.abs(img - ref)
    print(f"{W}^2 {nc}+{nf} ssaa {ssaa}: max {d.max():.2e} mean {d.mean():.2e}, {int(white.sum())} of {white.size} pixels white")
    _gate1(img, ref)
    for opt in ("skip_dead", "skip_empty", "certify_zero"):
        assert np.array_equal(R(**{opt: True}), img), opt
    for dtype in ("bf16x3", "f16x2"):
        _gate1(R(dtype=dtype), ref)
