"""Ray clipping on the CPU (include/nerf_mi355x.h, "ray clipping"): the NumPy restatement tests/helpers/ray_clip.py against an independent
float64 brute force and against hand-computed cases, and nerf_debug_clip_rays -- the function the kernel calls, run on the host --
against the restatement, bit for bit.  No GPU.

Measured when this test was written (3000 rays, 13 x 9 x 11 grid, 6 % occupancy): 0 hit mismatches, worst |dt| 0.18 of tol_r, 0
ambiguous rays, at most 30 walk rounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_clip as RC  # noqa: E402

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    """The issue's inputs, computed once: grid, rays, restatement, brute force."""
    bits = RC.random_grid(RC.GRID_DIMS, 0.06, seed=3)
    rays = RC.make_rays(RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS)
    out, hit, rounds = RC.clip_rays(bits, RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays["origins"], rays["dirs"], 0.0, 0.0, bounds=rays["bounds"],
                                    return_rounds=True)
    d = RC.directions(rays["dirs"])
    ref = RC.brute_force(bits, RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays["origins"], d, rays["bounds"][:, 0], rays["bounds"][:, 1])
    return dict(bits=bits, rays=rays, out=out, hit=hit, rounds=rounds, d=d, ref=ref)


def test_the_inputs_are_the_ones_asked_for(case):
    rays, d = case["rays"], case["rays"]["dirs"]
    assert d.shape == (3000, 3)
    zeros = (d == 0).sum(axis=1)
    assert ((zeros == 1) | (zeros == 2)).sum() == 250 and (zeros == 1).sum() > 50 and (zeros == 2).sum() > 50
    lo, step, dims = np.float64(RC.GRID_LO), np.float64(RC.GRID_STEP), np.float64(RC.GRID_DIMS)
    inside = np.all((rays["origins"] >= lo - 0.5 * step) & (rays["origins"] < lo + step * (dims - 0.5)), axis=1)
    assert 600 < inside.sum() < 2400
    short = rays["bounds"][:, 1] - rays["bounds"][:, 0] < 0.7
    assert 0.2 < short.mean() < 0.3
    occ = RC.unpack(case["bits"], RC.GRID_DIMS)
    assert 0.04 < occ.mean() < 0.08
    assert 0.2 < case["hit"].mean() < 0.95                                  # both outcomes are well represented


def test_restatement_against_the_float64_brute_force(case):
    rays, ref, out, hit = case["rays"], case["ref"], case["out"], case["hit"]
    tol_len = RC.tolerance(RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays["origins"], case["d"], ref["t_at_longest"])
    finite = np.isfinite(ref["longest"])          # -inf: with a zero direction component outside every occupied cell's slab -- a certain miss
    ambiguous = finite & (np.abs(ref["longest"]) <= 2.0 * np.where(finite, tol_len, 0.0))
    mismatch = (hit != ref["hit"]) & ~ambiguous
    both = hit & ref["hit"]
    worst = 0.0
    for k, key in enumerate(("t_first", "t_last")):
        tol = RC.tolerance(RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays["origins"], case["d"], ref[key])
        err = np.abs(out[:, k].astype(np.float64) - ref[key])
        worst = max(worst, float((err[both] / tol[both]).max()))
    print(f"hit mismatches {int(mismatch.sum())}, worst |dt| / tol {worst:.3f}, ambiguous {int(ambiguous.sum())} of {hit.size}, "
          f"hits {int(hit.sum())}, most rounds {int(case['rounds'].max())}")
    assert mismatch.sum() == 0, np.nonzero(mismatch)[0][:10]
    assert worst <= 1.0
    assert ambiguous.mean() <= 0.01
    assert case["rounds"].max() <= sum(RC.GRID_DIMS) + 3


def _one(bits, lo, step, dims, o, d, near, far, normalize=False):
    out, hit = RC.clip_rays(bits, lo, step, dims, np.float32([o]), np.float32([d]), near, far, normalize=normalize)
    return (float(out[0, 0]), float(out[0, 1])), bool(hit[0])


# a grid whose planes are exact in f32: lo = 0.5, step = 1 -> cell i spans [i, i + 1)
EX_LO, EX_STEP, EX_DIMS = (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (4, 3, 2)


def _grid(cells, dims=EX_DIMS):
    occ = np.zeros((dims[2], dims[1], dims[0]), bool)
    for x, y, z in cells:
        occ[z, y, x] = True
    return RC.pack(occ)


def test_hand_computed_cases(case):
    rays = case["rays"]
    # the empty grid hits nothing, and a miss returns its input bounds
    empty = RC.pack(np.zeros((11, 9, 13), bool))
    out, hit = RC.clip_rays(empty, RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays["origins"], rays["dirs"], 0.0, 0.0, bounds=rays["bounds"])
    assert not hit.any() and np.array_equal(_bits(out), _bits(rays["bounds"]))
    # the full grid: every ray whose [near, far] meets the box gets exactly {t_in, t_out} of the slab test
    full = RC.pack(np.ones((2, 3, 4), bool))
    assert _one(full, EX_LO, EX_STEP, EX_DIMS, (-2.0, 1.5, 0.5), (1.0, 0.0, 0.0), 0.0, 10.0) == ((2.0, 6.0), True)
    assert _one(full, EX_LO, EX_STEP, EX_DIMS, (-2.0, 1.5, 0.5), (1.0, 0.0, 0.0), 3.25, 4.5) == ((3.25, 4.5), True)
    assert _one(full, EX_LO, EX_STEP, EX_DIMS, (-2.0, 1.5, 0.5), (1.0, 0.0, 0.0), 0.0, 1.5) == ((0.0, 1.5), False)      # ends in front of the box
    assert _one(full, EX_LO, EX_STEP, EX_DIMS, (-2.0, 1.5, 0.5), (-1.0, 0.0, 0.0), 0.0, 10.0) == ((0.0, 10.0), False)   # points away
    assert _one(full, EX_LO, EX_STEP, EX_DIMS, (6.0, 2.5, 1.5), (-2.0, 0.0, 0.0), 0.0, 10.0) == ((1.0, 3.0), True)      # not unit, towards -x
    (a, b), h = _one(full, EX_LO, EX_STEP, EX_DIMS, (-1.0, -1.0, 1.0), (1.0, 1.0, 0.0), 0.0, 10.0)                      # along the diagonal: x, y in [0, 3)
    assert h and (a, b) == (1.0, 4.0)
    # a single occupied cell crossed along an axis gives the cell's two planes
    one = _grid([(2, 1, 0)])
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (-3.0, 1.5, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((5.0, 6.0), True)
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (2.5, 7.0, 0.25), (0.0, -1.0, 0.0), 0.0, 20.0) == ((5.0, 6.0), True)
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (2.5, 1.5, -4.0), (0.0, 0.0, 1.0), 0.0, 20.0) == ((4.0, 5.0), True)
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (-3.0, 2.5, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((0.0, 20.0), False)      # the row beside it
    # two cells with a gap: the span reaches from the first entry to the last exit
    two = _grid([(0, 1, 0), (3, 1, 0)])
    assert _one(two, EX_LO, EX_STEP, EX_DIMS, (-3.0, 1.5, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((3.0, 7.0), True)
    # a ray starting inside an occupied cell has t_first = near
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (2.25, 1.5, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((0.0, 0.75), True)
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (2.25, 1.5, 0.5), (1.0, 0.0, 0.0), 0.125, 0.5) == ((0.125, 0.5), True)
    # a ray lying exactly in a cell-boundary plane with d_y = 0 follows the half-open rule: y = 1 belongs to cell 1, y = 2 to cell 2
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (-3.0, 1.0, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((5.0, 6.0), True)
    assert _one(one, EX_LO, EX_STEP, EX_DIMS, (-3.0, 2.0, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((0.0, 20.0), False)
    # ... and on the grid's own faces: y = 0 is inside (G_lo <= o), y = 3 is not (o < G_hi)
    low = _grid([(2, 0, 0)])
    high = _grid([(2, 2, 0)])
    assert _one(low, EX_LO, EX_STEP, EX_DIMS, (-3.0, 0.0, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((5.0, 6.0), True)
    assert _one(high, EX_LO, EX_STEP, EX_DIMS, (-3.0, 3.0, 0.5), (1.0, 0.0, 0.0), 0.0, 20.0) == ((0.0, 20.0), False)


@pytest.mark.parametrize("dims", [(13, 9, 11), (33, 2, 1)])
@pytest.mark.parametrize("radius", [1, 2])
def test_dilation_against_maximum_filter(dims, radius):
    bits = RC.random_grid(dims, 0.03, seed=dims[0] + radius)
    occ = RC.unpack(bits, dims)
    # the maximum over every cell's (2 r + 1)^3 window of the zero-padded grid ...
    windows = np.lib.stride_tricks.sliding_window_view(np.pad(occ, radius), (2 * radius + 1,) * 3)
    want = windows.any(axis=(3, 4, 5))
    try:                                                                     # ... which is scipy's maximum filter, where scipy exists
        from scipy import ndimage
        assert np.array_equal(want, ndimage.maximum_filter(occ.astype(np.uint8), size=2 * radius + 1, mode="constant", cval=0).astype(bool))
    except ImportError:
        pass
    words, count, bounds = RC.dilate(bits, dims, radius)
    assert np.array_equal(RC.unpack(words, dims), want) and count == int(want.sum()) and bounds == RC.occupancy_bounds(want)
    assert want.sum() > occ.sum() > 0
    n = dims[0] * dims[1] * dims[2]
    if n % 32:
        assert int(words[-1]) >> (n % 32) == 0                               # the bits behind cell N - 1 are 0


def _debug(native, bits, lo, step, dims, rays, normalize=True, bounds=True, near=0.0, far=0.0):
    return native.clip_rays(None, bits, lo, step, dims, rays["origins"], rays["dirs"], near, far, bounds=rays["bounds"] if bounds else None,
                            normalize=normalize, return_count=True, debug_cpu=True)


def test_debug_clip_rays_is_the_restatement_bit_for_bit(native, case):
    rays = case["rays"]
    out, hit, count, refused = _debug(native, case["bits"], RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays)
    assert refused == 0 and count == int(case["hit"].sum())
    assert np.array_equal(hit, case["hit"]) and np.array_equal(_bits(out), _bits(case["out"]))
    # one origin for every ray, one [near, far] for every ray, directions taken as they are
    shared = dict(origins=rays["origins"][7], dirs=rays["dirs"], bounds=None)
    for normalize in (True, False):
        want = RC.clip_rays(case["bits"], RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, shared["origins"], shared["dirs"], 0.25, 3.0, normalize=normalize)
        out, hit, count, refused = _debug(native, case["bits"], RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, shared, normalize=normalize, bounds=False,
                                          near=0.25, far=3.0)
        assert refused == 0 and np.array_equal(hit, want[1]) and np.array_equal(_bits(out), _bits(want[0])) and count == int(want[1].sum())
    # the other grids of the GPU test, the empty and the full grid, and the exact grid of the hand-computed cases
    for dims, bits in (((33, 2, 1), RC.random_grid((33, 2, 1), 0.2, 5)), ((1, 1, 1), np.uint32([1])), ((40, 40, 40), RC.shell_grid()),
                       (RC.GRID_DIMS, RC.pack(np.zeros((11, 9, 13), bool))), (RC.GRID_DIMS, RC.pack(np.ones((11, 9, 13), bool)))):
        step = (0.21, 0.19, 0.17) if dims != (40, 40, 40) else (0.06, 0.06, 0.06)
        r = RC.make_rays(RC.GRID_LO, step, dims, n=700, n_zero=60, seed=dims[0])
        want = RC.clip_rays(bits, RC.GRID_LO, step, dims, r["origins"], r["dirs"], 0.0, 0.0, bounds=r["bounds"])
        out, hit, count, refused = _debug(native, bits, RC.GRID_LO, step, dims, r)
        assert refused == 0 and np.array_equal(hit, want[1]) and np.array_equal(_bits(out), _bits(want[0])), dims
        assert dims == RC.GRID_DIMS or 0 < hit.sum() < hit.size, dims
    one = _grid([(2, 1, 0)])
    o = np.float32([[-3.0, 1.0, 0.5], [-3.0, 2.0, 0.5], [2.25, 1.5, 0.5], [2.5, 7.0, 0.25]])
    d = np.float32([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, -1, 0]])
    out, hit, _, refused = native.clip_rays(None, one, EX_LO, EX_STEP, EX_DIMS, o, d, 0.0, 20.0, normalize=False, return_count=True, debug_cpu=True)
    assert refused == 0 and hit.tolist() == [True, False, True, True] and out.tolist() == [[5, 6], [0, 20], [0, 0.75], [5, 6]]


def test_non_finite_rays_stay_inside_the_grid_and_inside_themselves(native, case):
    """NaN / +-inf origins, directions and bounds: the call returns, the range check in front of the word load never has to turn an index
    away (so no cell outside the grid would have been read), and the rays beside them keep their bits."""
    rays = {k: v.copy() for k, v in case["rays"].items()}
    rng = np.random.default_rng(2)
    bad = np.sort(rng.choice(3000, 300, replace=False))
    specials = [np.nan, np.inf, -np.inf]
    for k, r in enumerate(bad):
        which = ("origins", "dirs", "bounds")[k % 3]
        col = rng.integers(0, rays[which].shape[1])
        rays[which][r, col] = specials[(k // 3) % 3]
        if k % 7 == 0:
            rays[which][r, :] = specials[(k // 7) % 3]
    for normalize in (True, False):
        clean = dict(case["rays"])
        want, want_hit, _, _ = _debug(native, case["bits"], RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, clean, normalize=normalize)
        out, hit, count, refused = _debug(native, case["bits"], RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays, normalize=normalize)
        assert refused == 0
        good = np.ones(3000, bool)
        good[bad] = False
        assert np.array_equal(hit[good], want_hit[good]) and np.array_equal(_bits(out[good]), _bits(want[good]))
        assert count == int(hit.sum())
    # the full grid, where every cell a stray index reaches would be "occupied"
    full = RC.pack(np.ones((11, 9, 13), bool))
    assert _debug(native, full, RC.GRID_LO, RC.GRID_STEP, RC.GRID_DIMS, rays)[3] == 0
