"""tests/helpers/surface_restatement.py checked on the CPU, before the GPU tests of the quantile depths and point clouds lean on it (no GPU):

  * against a float64 brute force on dyadic weights, whose partial sums are exact in float32: random rays, exact ties cum_i == q, and
    q = 1 on rays whose weights add up to exactly 1;
  * the edge cases of the contract: a NaN weight (nothing is reached at or behind it), all-zero rays, n = 1;
  * on the lego window of tests/test_normal_restatement_cpu.py (oracle networks, 20 + 50 samples): the median depth lies inside
    [near, far] and between the 0.25 and the 0.75 quantile depth wherever those are reached; on the silhouette rays (0.5 <= opacity <
    0.99) the median depth and depth / opacity differ -- they are different quantities;
  * the decidability condition of the oracle comparison in tests/test_gpu_surface.py: with the recorded ORACLE_MAX_CUM_DIFF at most a
    quarter of the rays that reach a quantile have a partial sum within twice that figure of it;
  * four mutants each change bits or indices: `>` for `>=`, a descending walk, t_{k+1} for t_k, and a keep test on `>`."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402
import surface_restatement as SR  # noqa: E402
from test_normal_restatement_cpu import LEGO_NORMALS  # noqa: E402  (the window, not its tests)

QS = (0.25, 0.5, 0.75)
# largest |cum_gpu - cum_oracle| over all samples of the LEGO_NORMALS window (GPU back end against oracle back end of restate_rays),
# measured on an MI355X on 2026-10-21 by tests/test_gpu_surface.py::test_quantile_depths_against_the_oracle, which asserts it at twice
# this figure.  A ray is DECIDED for q when no oracle cum_i lies within 2 D of q.
ORACLE_MAX_CUM_DIFF = 2.018e-05
MAX_UNDECIDED_SHARE = 0.25


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def brute_force(w, t, q):
    """float64: (depth, k) of one ray; k = -1 and depth 0 without a crossing."""
    cum = 0.0
    for i in range(len(w)):
        cum += float(w[i])
        if cum >= float(q):
            return float(t[i]), i
    return 0.0, -1


def dyadic_rays(rng, R, n, total=1024):
    """Weights that are multiples of 2^-10 with a sum <= 1: every partial sum is exact in float32 (and in float64)."""
    parts = rng.integers(0, 40, (R, n))
    parts[rng.random((R, n)) < 0.5] = 0                               # empty space
    scale = np.minimum(1.0, total / np.maximum(parts.sum(axis=1), 1))
    parts = np.floor(parts * scale[:, None]).astype(np.int64)
    assert (parts.sum(axis=1) <= total).all()
    t = np.sort(rng.uniform(2.0, 6.0, (R, n)), axis=1).astype(np.float32)
    return (parts / float(total)).astype(np.float32), t, parts


@pytest.mark.parametrize("n", [1, 8, 16, 17, 70])
def test_quantile_depths_against_float64(n):
    rng = np.random.default_rng(100 + n)
    w, t, parts = dyadic_rays(rng, 97, n)
    w[5] = 0.0                                                         # an all-zero ray
    # exact ties: the quantile IS a partial sum of ray 0 / ray 1; and thresholds no sum can hit exactly
    cum0 = np.cumsum(parts[0]) / 1024.0
    ties = [float(c) for c in np.unique(cum0) if 0 < c <= 1][:2]
    qs = np.float32(ties + [0.125, 0.5, 0.3, 1.0][: 8 - len(ties)])
    depth, index = SR.quantile_depths(w, t, qs, return_index=True)
    assert depth.shape == (len(qs), 97) and depth.dtype == np.float32
    for j, q in enumerate(qs):
        for r in range(97):
            d, k = brute_force(w[r], t[r], q)
            assert index[j, r] == k and _bits(depth[j, r]) == _bits(np.float32(d)), (j, r, q)
    for c in ties:                                                     # the tie is reached AT the sample whose sum equals q, not one later
        j = list(qs).index(np.float32(c))
        assert cum0[index[j, 0]] == c
    assert (index[:, 5] == -1).all() and (_bits(depth[:, 5]) == 0).all()


def test_q_equal_one_on_a_sum_of_exactly_one():
    w = np.float32([[0.25, 0.0, 0.5, 0.25, 0.0], [0.25, 0.0, 0.5, 0.125, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0]])
    t = np.tile(np.float32([2.0, 3.0, 4.0, 5.0, 5.5]), (3, 1))
    depth, index = SR.quantile_depths(w, t, [1.0, 0.75], return_index=True)
    assert index.tolist() == [[3, -1, 0], [2, 2, 0]]
    assert depth.tolist() == [[5.0, 0.0, 2.0], [4.0, 4.0, 2.0]]
    assert np.array_equal(SR.cumulative(w)[:, -1], np.float32([1.0, 0.875, 1.0]))


def test_nan_weight_and_single_sample():
    w = np.float32([[0.25, np.nan, 0.5, 0.25], [0.5, 0.25, np.nan, 0.25]])
    t = np.tile(np.float32([2.0, 3.0, 4.0, 5.0]), (2, 1))
    depth, index = SR.quantile_depths(w, t, [0.25, 0.5, 0.75], return_index=True)
    assert index.tolist() == [[0, 0], [-1, 0], [-1, 1]]                # behind the NaN the sum is NaN: never reached
    assert depth.tolist() == [[2.0, 2.0], [0.0, 2.0], [0.0, 3.0]]
    depth, index = SR.quantile_depths(np.float32([[0.6], [0.4], [0.0]]), np.float32([[3.5], [3.5], [3.5]]), [0.5], return_index=True)
    assert index.tolist() == [[0, -1, -1]] and depth.tolist() == [[3.5, 0.0, 0.0]]


def test_points_keep_rule_and_records():
    o = np.float32([[0, 0, 4], [1, 0, 4], [2, 0, 4], [3, 0, 4], [4, 0, 4]])
    d = np.tile(np.float32([0, 0, -1]), (5, 1))
    dq = np.float32([3.0, 0.0, 2.5, 3.5, 2.0])
    A = np.float32([0.9, 0.9, 0.5, 0.4, np.nan])
    Cc = np.float32([[0.45, 0.9, 0.0], [1, 1, 1], [0.25, 0.5, 0.125], [0.1, 0.1, 0.1], [0.5, 0.5, 0.5]])
    nrm = np.arange(15, dtype=np.float32).reshape(5, 3)
    p = SR.points(o, d, dq, Cc, A, nrm, 0.5)
    assert p["n"] == 2 and p["ray"].tolist() == [0, 2]                  # ray 1: no crossing; ray 3: too transparent; ray 4: NaN opacity
    assert p["xyz"].tolist() == [[0.0, 0.0, 1.0], [2.0, 0.0, 1.5]]
    assert np.array_equal(_bits(p["rgb"]), _bits(np.float32([[0.45, 0.9, 0.0], [0.25, 0.5, 0.125]]) / np.float32([[0.9], [0.5]])))
    assert p["normals"].tolist() == nrm[[0, 2]].tolist() and p["depth"].tolist() == [3.0, 2.5] and p["opacity"].tolist() == [np.float32(0.9), 0.5]
    assert SR.points(o[0], d, dq, Cc, A, None, 0.0)["ray"].tolist() == [0, 2, 3] and "normals" not in SR.points(o[0], d, dq, Cc, A, None, 0.0)
    assert SR.points(o, d, dq, Cc, A, nrm, 1.0)["n"] == 0
    # mutant: a keep test on `>` drops the ray that sits exactly on the threshold
    assert SR.points(o, d, dq, Cc, A, nrm, 0.5, strict_keep=True)["ray"].tolist() == [0]


# ---- the lego window ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lego(oracle, oracle_nets, samples):
    P = LEGO_NORMALS
    be = RR.OracleBackend(oracle, *oracle_nets)
    cam = oracle.camera_from_samples(samples, P["W"], P["W"])
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, P["crop"])
    rs = RB.restate_rays(be, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    depth, index = SR.quantile_depths(rs["w_fine"], rs["t_fine"], QS, return_index=True)
    return dict(rs=rs, near=near, far=far, depth=depth, index=index, origin=origin)


def test_lego_median_depth_is_ordered_and_inside_the_bounds(lego):
    rs, depth, index = lego["rs"], lego["depth"], lego["index"]
    assert np.array_equal(_bits(SR.cumulative(rs["w_fine"])[:, -1]), _bits(rs["opacity"]))      # the last partial sum IS the opacity
    for j, q in enumerate(QS):
        reached = index[j] >= 0
        assert np.array_equal(reached, rs["opacity"] >= np.float32(q))
        assert (_bits(depth[j][~reached]) == 0).all()
        assert (depth[j][reached] >= lego["near"]).all() and (depth[j][reached] <= lego["far"]).all()
    r75 = index[2] >= 0
    assert r75.sum() >= 100
    assert (depth[0][r75] <= depth[1][r75]).all() and (depth[1][r75] <= depth[2][r75]).all()
    assert (depth[0][r75] < depth[2][r75]).any()


def test_lego_silhouette_median_is_not_the_expected_depth(lego):
    """On the rays that are absorbed partly by the model and partly behind it the two depths are different quantities."""
    rs = lego["rs"]
    edge = (rs["opacity"] >= 0.5) & (rs["opacity"] < 0.99)
    assert edge.sum() >= 3, int(edge.sum())
    expected = rs["depth"][edge] / rs["opacity"][edge]
    median = lego["depth"][1][edge]
    print(f"\n{int(edge.sum())} silhouette rays: |median - depth / opacity| from {np.abs(median - expected).min():.4f} to {np.abs(median - expected).max():.4f}")
    # obtained: 15 rays, differences from 0.0006 to 0.065.  An ulp of these depths is 2.4e-7: a difference of 1e-4 on every ray, and of
    # more than 0.01 on some, is not a rounding of one quantity
    assert (np.abs(median - expected) > 1e-4).all() and np.abs(median - expected).max() > 0.01


def undecided_share(cum, opacity, q, D):
    """Of the rays with opacity >= q, the share with an oracle partial sum within 2 D of q."""
    reach = opacity >= np.float32(q)
    near = (np.abs(cum.astype(np.float64) - float(np.float32(q))) <= 2.0 * D).any(axis=1)
    return float((near & reach).sum()) / max(int(reach.sum()), 1), int(reach.sum())


def test_lego_window_decides_most_rays(lego):
    assert ORACLE_MAX_CUM_DIFF is not None, "measure D on an MI355X (tests/test_gpu_surface.py prints it) and record it"
    cum = SR.cumulative(lego["rs"]["w_fine"])
    for q in QS:
        share, n = undecided_share(cum, lego["rs"]["opacity"], q, ORACLE_MAX_CUM_DIFF)
        print(f"\nq = {q}: {share:.3f} of {n} rays undecided at D = {ORACLE_MAX_CUM_DIFF:.3e}")
        assert n >= 100 and share <= MAX_UNDECIDED_SHARE, (q, share)


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def test_mutant_strict_comparison_moves_the_ties():
    w = np.float32([[0.25, 0.25, 0.25, 0.25]])
    t = np.float32([[2.0, 3.0, 4.0, 5.0]])
    assert SR.quantile_depths(w, t, [0.5, 1.0]).tolist() == [[3.0], [5.0]]
    assert SR.quantile_depths(w, t, [0.5, 1.0], strict=True).tolist() == [[4.0], [0.0]]


def test_mutant_descending_walk_changes_indices(lego):
    rs = lego["rs"]
    _, index = SR.quantile_depths(rs["w_fine"], rs["t_fine"], QS, return_index=True, descending=True)
    # A thin, opaque surface absorbs the ray within a sample or two, and the walk from the back then crosses q at the same sample: obtained,
    # 13 of the 112 rays that reach the median change their index.  One changed ray is what a bit-for-bit comparison needs.
    for j in range(len(QS)):
        hit = lego["index"][j] >= 0
        changed = index[j][hit] != lego["index"][j][hit]
        print(f"\nq = {QS[j]}: the descending walk moves {int(changed.sum())} of {int(hit.sum())} crossings")
        assert changed.sum() >= 1


def test_mutant_next_sample_changes_bits(lego):
    rs = lego["rs"]
    depth = SR.quantile_depths(rs["w_fine"], rs["t_fine"], QS, next_sample=True)
    hit = lego["index"][1] >= 0
    assert (_bits(depth[1][hit]) != _bits(lego["depth"][1][hit])).mean() >= 0.9
