"""The NumPy restatement of the isosurface extraction (tests/helpers/marching_tets.py) is fit for purpose: on the synthetic fields it passes the
invariants that tests/test_gpu_mesh.py then transfers to the GPU by demanding bit-equality with it -- every vertex on its edge, closed
fields manifold and consistently wound, the right Euler characteristic, positive volume and outward triangle normals.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import marching_tets as MT  # noqa: E402

F = np.float32
DIMS = [(3, 3, 3), (9, 7, 5), (17, 9, 5), (33, 7, 3), (24, 22, 19)]
FINE = (24, 22, 19)        # steps 0.087 .. 0.111: every feature of the closed fields (smallest: the torus tube, radius 0.26) spans several cells


def _mesh(field, dims, **kw):
    lo, step = MT.unit_lattice(dims)
    sigma = field(lo, step, dims, **kw)
    return (lo, step, sigma) + MT.marching_tets(sigma, lo, step, 0.0)


def _border_below(sigma, iso=0.0):
    b = np.ones(sigma.shape, bool)
    b[1:-1, 1:-1, 1:-1] = False
    return bool((sigma[b] < iso).all())


@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_vertices_lie_on_their_edges(dims):
    lo, step, sigma, v, n, t = _mesh(MT.sphere_field, dims)
    a, b = MT.vertex_edges(sigma, 0.0)
    assert len(v) == len(a) > 0
    ax = MT.lattice_axes(lo, step, dims)
    pa = np.stack([ax[k][a[:, k]] for k in range(3)], axis=1).astype(np.float64)
    pb = np.stack([ax[k][b[:, k]] for k in range(3)], axis=1).astype(np.float64)
    lo_box, hi_box = np.minimum(pa, pb), np.maximum(pa, pb)
    assert ((v >= lo_box - 1e-6) & (v <= hi_box + 1e-6)).all()                 # inside the edge's box ...
    off = np.cross(pb - pa, v - pa)
    assert np.abs(off).max() <= 1e-6                                          # ... and on its line
    r = np.linalg.norm(v.astype(np.float64) - np.array([0.03, -0.02, 0.05]), axis=1)
    assert (np.abs(r - 0.71) <= np.linalg.norm(pb - pa, axis=1) + 1e-6).all()  # the true crossing lies on the same edge
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5                # unit normals, pointing away from the centre
    assert (np.einsum("ij,ij->i", n, v - F([0.03, -0.02, 0.05])) > 0).all()


@pytest.mark.parametrize("field", [MT.sphere_field, MT.two_spheres_field, MT.torus_field], ids=lambda f: f.__name__)
@pytest.mark.parametrize("dims", DIMS, ids=str)
def test_closed_fields_are_manifold_and_wound_outwards(field, dims):
    lo, step, sigma, v, n, t = _mesh(field, dims)
    assert _border_below(sigma)
    if len(t) == 0:
        assert not (sigma > 0).any()                         # a lattice too coarse to catch the field: nothing inside, nothing emitted
        return
    assert MT.is_closed_manifold(t)
    assert (np.sort(t, axis=1)[:, 0] == t[:, 0]).all()       # canonical form: the smallest id first
    assert MT.signed_volume(v, t) > 0


@pytest.mark.parametrize("field,chi", [(MT.sphere_field, 2), (MT.two_spheres_field, 4), (MT.torus_field, 0)], ids=["sphere", "two spheres", "torus"])
def test_euler_characteristic(field, chi):
    lo, step, sigma, v, n, t = _mesh(field, FINE)
    assert MT.is_closed_manifold(t) and MT.euler_characteristic(len(v), t) == chi


def _analytic_outward(name, c):
    """-grad sigma at the points c (float64), for the fields of marching_tets.py."""
    if name == "sphere":
        d = c - np.array([0.03, -0.02, 0.05])
    elif name == "plane":
        return np.tile(np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81]), (len(c), 1))
    elif name == "torus":
        q = c[:, :2] - np.array([0.01, -0.02])
        rho = np.linalg.norm(q, axis=1)
        ring = q / rho[:, None] * 0.6                         # nearest point of the centre circle
        d = c - np.concatenate([ring + np.array([0.01, -0.02]), np.full((len(c), 1), 0.015)], axis=1)
    return d / np.linalg.norm(d, axis=1)[:, None]


@pytest.mark.parametrize("name,field", [("sphere", MT.sphere_field), ("plane", MT.plane_field), ("torus", MT.torus_field)])
def test_triangle_normals_point_towards_lower_density(name, field):
    lo, step, sigma, v, n, t = _mesh(field, FINE)
    tn, c = MT.triangle_normals_and_centroids(v, t)
    dots = np.einsum("ij,ij->i", tn, _analytic_outward(name, c))
    assert len(t) > 100 and (dots > 0).all(), (int((dots <= 0).sum()), dots.min())


def test_mirrored_lattice_has_the_same_triangles():
    """Winding lives in index space: reversing an axis of the lattice (negative step, the field mirrored with it) leaves the index-space
    problem untouched, so the triangle array is the same and only the positions are mirrored."""
    dims = (9, 7, 5)
    lo, step = MT.unit_lattice(dims)
    sigma = MT.sphere_field(lo, step, dims)
    v, n, t = MT.marching_tets(sigma, lo, step, 0.0)
    hi = (lo + step * (F(dims) - 1)).astype(F)
    lo2, step2 = F([hi[0], lo[1], lo[2]]), F([-step[0], step[1], step[2]])
    v2, n2, t2 = MT.marching_tets(sigma, lo2, step2, 0.0)
    assert np.array_equal(t, t2) and len(t) > 0
    assert MT.signed_volume(v, t) > 0 > MT.signed_volume(v2, t2)              # one negative step: wound inwards in world space


def test_equal_to_iso_nan_and_inf():
    dims = (9, 9, 9)
    sigma = MT.integer_field(dims)                           # the level set passes through the lattice point (6, 5, 5) and its mirror images
    assert (sigma == 0).any() and sigma.max() > 0 > sigma.min()
    lo, step = F([0, 0, 0]), F([1, 1, 1])
    v, n, t = MT.marching_tets(sigma, lo, step, 0.0)
    assert MT.is_closed_manifold(t) and MT.euler_characteristic(len(v), t) == 2     # in index terms, even where positions coincide
    assert len(np.unique(v, axis=0)) < len(v)                                     # sigma == iso at a corner: several edges meet in one position
    for bad in (np.nan, np.inf):
        s = sigma.copy(); s[4, 4, 6] = bad
        v2, n2, t2 = MT.marching_tets(s, lo, step, 0.0)
        assert np.isfinite(v2).all() and 0 < len(t2) < len(t) and not MT.is_closed_manifold(t2)   # the cells around it are skipped: a hole
    below = np.full((3, 4, 5), -1, F)
    for s in (below, -below):
        v0, n0, t0 = MT.marching_tets(s, lo, step, 0.0)
        assert v0.shape == (0, 3) and n0.shape == (0, 3) and t0.shape == (0, 3)
