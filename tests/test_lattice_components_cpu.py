"""The restatement tests/helpers/lattice_components.py is fit for purpose (no device): it equals scipy.ndimage.label with the 14-neighbour
structure where scipy imports (skipped, visibly, where it does not), and -- independently of scipy -- it reproduces hand-counted lattices, the diagonal / anti-diagonal rule and the
tie order; filter_mesh is the identity for keep-all, yields a closed manifold of Euler characteristic 2 for the largest of two spheres, and
never leaves a triangle that references a dropped vertex."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lattice_components as LC  # noqa: E402
import marching_tets as MT  # noqa: E402

F = np.float32
LATTICES = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (9, 7, 5), (33, 7, 3), (40, 30, 29)]
FIELDS = {
    "floaters": LC.floaters,
    "snake": LC.snake,
    "hollow": LC.hollow,
    "noise12": lambda dims: LC.noise(dims, 0.12, 1),
    "noise20": lambda dims: LC.noise(dims, 0.2, 2),
    "all_inside": lambda dims: np.ones(dims[::-1], F),
    "all_outside": lambda dims: np.zeros(dims[::-1], F),
}


@functools.lru_cache(maxsize=None)
def _case(field, dims):
    sigma = FIELDS[field](dims)
    labels, table = LC.components(sigma, 0.0)
    sigma.setflags(write=False); labels.setflags(write=False)
    return sigma, labels, table


def _check_table(sigma, labels, table):
    """What the definition says about a table, checked with plain NumPy on the labels."""
    ins = LC.inside_mask(sigma, 0.0)
    assert ((labels != LC.NONE) == ins).all()
    nz, ny, nx = sigma.shape
    lin = np.arange(nz * ny * nx, dtype=np.int64).reshape(sigma.shape)
    assert sorted(e[0] for e in table) == sorted(np.unique(labels[ins]).tolist())
    assert [(-e[1], e[0]) for e in table] == sorted((-e[1], e[0]) for e in table)
    for label, n_points, bounds in table[:40]:
        pts = labels == label
        assert n_points == int(pts.sum()) and label == int(lin[pts].min())
        iz, iy, ix = np.nonzero(pts)
        assert bounds == (ix.min(), iy.min(), iz.min(), ix.max(), iy.max(), iz.max())


@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("field", list(FIELDS))
def test_restatement_meets_the_definition(field, dims):
    sigma, labels, table = _case(field, dims)
    _check_table(sigma, labels, table)


@pytest.mark.parametrize("dims", LATTICES, ids=str)
@pytest.mark.parametrize("field", list(FIELDS))
def test_restatement_equals_scipy(field, dims):
    ndimage = pytest.importorskip("scipy.ndimage")                 # reported as skipped where scipy is missing: the comparison did not run
    sigma, labels, table = _case(field, dims)
    structure = np.zeros((3, 3, 3), bool)                        # axes (z, y, x)
    structure[1, 1, 1] = True
    for dx, dy, dz in LC.NEIGHBOURS:
        structure[1 + dz, 1 + dy, 1 + dx] = True
    assert structure.sum() == 15
    lab, count = ndimage.label(LC.inside_mask(sigma, 0.0), structure=structure)
    assert count == len(table)
    lin = np.arange(sigma.size, dtype=np.int64).reshape(sigma.shape)
    want = np.full(sigma.shape, LC.NONE, np.uint32)
    if count:
        mins = ndimage.minimum(lin, lab, index=np.arange(1, count + 1)).astype(np.int64)
        want[lab > 0] = mins[lab[lab > 0] - 1]
    assert np.array_equal(labels, want)


def test_the_noise_fields_are_what_the_gpu_tests_need():
    _, _, t12 = _case("noise12", (40, 30, 29))
    _, _, t20 = _case("noise20", (40, 30, 29))
    print(f"\nnoise 0.12: {len(t12)} components, largest {[e[1] for e in t12[:6]]}; noise 0.2: {len(t20)} components, largest {[e[1] for e in t20[:4]]}")
    assert len(t12) > 500 and len(t20) > 100
    sizes = [e[1] for e in t12[:64]]
    assert len(set(sizes)) < len(sizes)                            # ties among the first 64
    assert t20[0][1] > 20 * t20[1][1]                              # one large component beside small ones


def test_hand_counted_lattices():
    s = np.zeros((3, 3, 4), F)                                     # (nz, ny, nx) = (3, 3, 4): index = ix + 4 (iy + 3 iz)
    s[0, 0, 0] = s[0, 0, 1] = s[0, 1, 1] = 1                       # an L of three points: indices 0, 1, 5
    s[2, 2, 3] = 1                                                 # a single point: index 35
    s[1, 0, 3] = s[2, 1, 3] = 1                                    # (3,0,1) and (3,1,2): differ by (0,1,1), a Kuhn face diagonal: indices 15, 31
    labels, table = LC.components(s, 0.0)
    assert table == [(0, 3, (0, 0, 0, 1, 1, 0)), (15, 3, (3, 0, 1, 3, 2, 2))]      # (3,1,2)-(3,2,2) are axis neighbours: 15, 31, 35 are one piece
    assert labels[0, 1, 1] == 0 and labels[2, 2, 3] == 15 and labels[1, 1, 1] == LC.NONE
    s[2, 1, 3] = 0                                                 # cut it: 15 and 35 are alone, ranked after the L, by label
    assert LC.components(s, 0.0)[1] == [(0, 3, (0, 0, 0, 1, 1, 0)), (15, 1, (3, 0, 1, 3, 0, 1)), (35, 1, (3, 2, 2, 3, 2, 2))]


def test_body_diagonal_joins_and_anti_diagonal_does_not():
    s = np.zeros((2, 2, 2), F)
    s[0, 0, 0] = s[1, 1, 1] = 1                                    # (0,0,0)-(1,1,1)
    assert [e[:2] for e in LC.components(s, 0.0)[1]] == [(0, 2)]
    s = np.zeros((2, 2, 2), F)
    s[0, 0, 1] = s[0, 1, 0] = 1                                    # (1,0,0)-(0,1,0)
    assert [e[:2] for e in LC.components(s, 0.0)[1]] == [(1, 1), (2, 1)]
    for a, b, joined in (((0, 0, 0), (1, 1, 0), True), ((0, 0, 0), (1, 0, 1), True), ((0, 0, 0), (0, 1, 1), True),
                         ((1, 0, 0), (0, 0, 1), False), ((0, 1, 0), (0, 0, 1), False), ((1, 1, 0), (0, 0, 1), False), ((1, 0, 1), (0, 1, 0), False)):
        s = np.zeros((2, 2, 2), F)
        s[a[2], a[1], a[0]] = s[b[2], b[1], b[0]] = 1
        assert (len(LC.components(s, 0.0)[1]) == 1) == joined, (a, b)


def test_tie_order_and_filters():
    sigma, labels, table = _case("floaters", (40, 30, 29))
    sizes = [e[1] for e in table]
    print(f"\nfloaters: sizes {sizes}, labels {[e[0] for e in table]}")
    assert len(table) == 9 and sizes[2] == sizes[3] and table[2][0] < table[3][0]          # the two equal blobs, smaller label first
    assert sizes[0] > sizes[1] > sizes[2] and sizes[3] > sizes[4] > sizes[5] == 2 and sizes[6:] == [1, 1, 1]
    assert [e[0] for e in table[6:]] == sorted(e[0] for e in table[6:])
    assert LC.kept_labels(table, 3, 0) == [e[0] for e in table[:3]]                         # crosses the tie
    assert LC.kept_labels(table, 0, sizes[4]) == [e[0] for e in table[:5]]
    assert LC.kept_labels(table, 2, sizes[4]) == [e[0] for e in table[:2]]
    assert LC.kept_labels(table, 64, 10 ** 6) == [] and len(LC.kept_labels(table, 0, 0)) == 9
    diag = labels[24, 3, 3]
    assert diag == labels[25, 4, 4] != LC.NONE and labels[3, 26, 36] != labels[3, 27, 35]   # joined by the body diagonal; apart across the anti-diagonal


def test_nan_is_never_labelled_and_inf_is():
    s = LC.floaters((40, 30, 29)).copy()
    s[14, 15, 15] = np.nan                                         # inside the sphere
    s[0, 0, 0] = np.nan
    s[28, 29, 39] = np.inf
    s[10, 2, 2] = -np.inf
    labels, table = LC.components(s, 0.0)
    assert labels[14, 15, 15] == LC.NONE and labels[0, 0, 0] == LC.NONE and labels[10, 2, 2] == LC.NONE
    assert labels[28, 29, 39] == 39 + 40 * (29 + 30 * 28) and len(table) == 10


@functools.lru_cache(maxsize=None)
def _mesh(field, dims):
    lo, step = MT.unit_lattice(dims)
    sigma = MT.two_spheres_field(lo, step, dims) if field == "two_spheres" else FIELDS[field](dims)
    return (sigma,) + MT.marching_tets(sigma, lo, step, 0.0)


@pytest.mark.parametrize("field", ["two_spheres", "floaters", "hollow", "noise20"])
def test_filter_mesh(field):
    sigma, v, n, t = _mesh(field, (40, 30, 29))
    fv, fn, ft, n_comp, n_kept = LC.filter_mesh(sigma, 0.0, v, n, t, 0, 0)                   # keep-all: the identity
    assert n_kept == n_comp and np.array_equal(fv.view(np.uint32), v.view(np.uint32)) and np.array_equal(fn.view(np.uint32), n.view(np.uint32))
    assert np.array_equal(ft, t)
    fv, fn, ft, n_comp, n_kept = LC.filter_mesh(sigma, 0.0, v, n, t, 1, 0)
    assert n_kept == 1 and 0 < len(ft) and len(fv) > 0 and ft.max() == len(fv) - 1           # no triangle references a dropped vertex
    if n_comp > 1:
        assert len(ft) < len(t) and len(fv) < len(v)
    if field == "two_spheres":
        assert n_comp == 2 and MT.is_closed_manifold(ft) and MT.euler_characteristic(len(fv), ft) == 2
        assert MT.euler_characteristic(len(v), t) == 4
    if field == "hollow":
        assert n_comp == 1 and MT.is_closed_manifold(ft) and MT.euler_characteristic(len(fv), ft) == 4      # two spheres' worth of surface, both kept
    fv0, _, ft0, _, n_kept0 = LC.filter_mesh(sigma, 0.0, v, n, t, 64, 10 ** 6)                # keeps nothing
    assert (len(fv0), len(ft0), n_kept0) == (0, 0, 0)
