"""The inputs of tests/test_gpu_sampling_shapes.py (tests/helpers/sampling_cases.py) are fit for purpose -- shown with the CPU oracle
alone, so that the GPU tests' exclusions and exact comparisons rest on something that is checked:
  * every family is finite; the density family holds empty, partly absorbing and terminated rays at every sample count used;
  * one-hot rays give exactly one-hot weights and exactly the chosen sample's colour (pure white when empty) in the oracle, so a
    bit-exact comparison of the kernels on them is legitimate;
  * the oracle's f32 weights stay within the project's 2e-6 of a float64 evaluation of the same recurrence at every count (up to 1070
    samples per ray), so 2e-6 is not used up by the reference's own rounding on long rays;
  * near-cut rays -- whose float64 transmittance comes within a relative 1e-3 of the 1e-4 cut at or before the cut, where one ulp of expf
    may move the cut by a sample -- are the only rays the GPU tests leave out of their weight comparisons: at most 2 % of a family.
    The cap is a condition on the generator: if a seed breaks it, the seed changes, not the cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sampling_cases as S

W_TOL = 2e-6
# (sample count, rays) of every use in the GPU tests: resample shapes at RESAMPLE_RAYS rays, composite counts at up to 130 rays
USES = sorted({(nc, S.RESAMPLE_RAYS) for nc, _ in S.RESAMPLE_SHAPES} | {(n, max(S.COMPOSITE_RAYS)) for n in S.COMPOSITE_N})


@pytest.fixture(scope="module")
def families(oracle):
    """{(family, n, R): (t, sigma, oracle weights, float64 weights, near_cut, terminated)}, computed once"""
    out = {}
    for name, gen in S.FAMILIES.items():
        for n, R in USES:
            t, s = gen(oracle, R, n)
            w = np.stack([oracle.compute_weights(s[r], t[r], S.FAR) for r in range(R)])
            m = [S.weights_f64(s[r], t[r]) for r in range(R)]
            out[name, n, R] = (t, s, w, np.stack([x[0] for x in m]), np.array([x[1] for x in m]), np.array([x[2] for x in m]))
    return out


def test_families_are_finite_and_ordered(families):
    for (name, n, R), (t, s, w, w64, _, _) in families.items():
        assert t.shape == s.shape == (R, n) and t.dtype == s.dtype == np.float32
        assert np.isfinite(t).all() and np.isfinite(s).all() and np.isfinite(w).all() and (s >= 0).all()
        assert np.all(np.diff(t, axis=1) >= 0) and t.min() >= S.NEAR and t.max() <= S.FAR
        if name == "duplicate" and n >= 2:
            assert np.all((np.diff(t, axis=1) == 0).any(axis=1))      # every ray has a zero-width interval
        else:
            assert np.all(np.diff(t, axis=1) > 0)


def test_density_family_mixes_empty_partial_and_terminated_rays(families):
    for n, R in USES:
        _, _, w, _, near, term = families["density", n, R]
        empty = (w == 0).all(axis=1)
        partial = ~empty & ~term & ~near
        assert empty.any() and partial.any() and (term & ~near).any(), (n, R, empty.sum(), partial.sum(), term.sum())
        # a terminated ray of more than one sample has its zero-filled tail (src/lib.rs:276-279) unless the cut came at the last sample
        if n >= 16:
            assert (w[term][:, -1] == 0).any()


def test_one_hot_rays_are_exact_in_the_oracle(oracle):
    for n, R in USES:
        t, s, k = S.one_hot_rays(oracle, R, n, offset=n)
        col = S.distinct_colours(R, n)
        for r in range(R):
            w = oracle.compute_weights(s[r], t[r], S.FAR)
            rgb = oracle.integrate_ray(col[r], s[r], t[r], S.FAR)
            if k[r] == n:
                assert not w.any() and np.all(rgb == 1.0)                  # empty ray: pure white
            else:
                assert w[k[r]] == 1.0 and np.count_nonzero(w) == 1         # exactly one-hot
                assert np.array_equal(rgb, col[r, k[r]])                   # exactly that sample's colour
    # the positions cover 0, the last sample, an empty ray and both sides of every multiple of 16 (and so of 64)
    ks = S.one_hot_positions(1070)
    assert {0, 1069, 1070, 15, 16, 63, 64, 1023, 1024, 1055, 1056} <= set(ks)


def test_oracle_weights_match_the_float64_model(families):
    worst = 0.0
    for (name, n, R), (_, _, w, w64, near, _) in families.items():
        d = np.abs(w.astype(np.float64) - w64)[~near]
        if d.size:
            worst = max(worst, float(d.max()))
            assert d.max() <= W_TOL, (name, n, d.max())
    print(f"\noracle f32 weights vs float64 model: max |dw| = {worst:.2e}")


def test_near_cut_rays_are_rare(families):
    for name in S.FAMILIES:
        near = np.concatenate([v[4] for k, v in families.items() if k[0] == name])
        print(f"\n{name}: {int(near.sum())} near-cut rays of {near.size}")
        assert near.mean() <= 0.02


def test_explicit_uniforms_cover_edges_and_misses(oracle):
    """With enough draws a ray's uniforms hold every special value; with few, neighbouring rays hold them together."""
    t, s = S.density_rays(oracle, 1, 20)
    _, cdf = oracle.sample_importance_u(np.zeros(1, np.float32), t[0], oracle.compute_weights(s[0], t[0], S.FAR))
    assert cdf[0] == 0.0 and cdf[-1] == 1.0 and np.all(np.diff(cdf) > 0)
    want = set(np.concatenate([[0.0, S.U_MAX, 1.0, -0.5, 2.0], cdf, np.nextafter(cdf, np.float32(-np.inf))]).astype(np.float32).tolist())
    u = S.explicit_uniforms(cdf, 64)
    assert u.shape == (64,) and u.dtype == np.float32 and want <= set(u.tolist())
    few = np.concatenate([S.explicit_uniforms(cdf, 5, r) for r in range(S.RESAMPLE_RAYS)])
    assert len(few) == 45 and set(few.tolist()) == want      # 43 entries, 45 draws: the list wraps round
    assert S.explicit_uniforms(cdf, 1).shape == (1,)


def test_wide_ratio_rays_tell_the_bins_of_an_edge_draw_apart(oracle):
    """On evenly spaced samples a draw on a bin edge gives the same float from the bin above and from the bin below it (the lerp ends
    where the next begins, exactly); the wide-ratio family has edges where it does not, at every count used -- and no near-cut ray."""
    for family in S.FAMILIES:
        for nc, _ in S.RESAMPLE_SHAPES:
            assert not S.edges_that_tell_bins_apart(S.FAMILIES[family](oracle, S.RESAMPLE_RAYS, nc)[0]).any(), (family, nc)
    for nc in S.WIDE_NC:
        t, s = S.wide_ratio_rays(S.RESAMPLE_RAYS, nc)
        assert np.isfinite(t).all() and np.isfinite(s).all() and np.all(np.diff(t, axis=1) > 0) and t.min() > 1e-30
        w = np.stack([oracle.compute_weights(s[r], t[r], S.FAR) for r in range(len(t))])
        w64 = np.stack([S.weights_f64(s[r], t[r])[0] for r in range(len(t))])
        assert np.isfinite(w).all() and np.abs(w - w64).max() <= W_TOL and not S.near_cut_mask(s, t).any()
        tell = S.edges_that_tell_bins_apart(t)
        print(f"\nwide-ratio nc = {nc}: {int(tell.sum())} of {tell.size} interior edges tell the bins apart")
        assert tell.any()
