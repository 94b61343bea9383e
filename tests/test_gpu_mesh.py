"""Isosurface meshes on the GPU: nerf_isosurface_grid (marching tetrahedra on a caller's sigma lattice) and nerf_extract_mesh (the same kernels
on a lattice the context evaluates itself, plus vertex colours), against the NumPy restatement tests/helpers/marching_tets.py.

Stated tolerances: none.  The header fixes every operation and its rounding, the restatement follows it with one float32 NumPy operation per
rounding, so vertices, normals, triangles and counts must agree BIT FOR BIT; the network entry points must equal nerf_isosurface_grid on
nerf_density_grid's sigma, and the colours nerf_forward_batch at the vertices, bit for bit as well.  The geometric invariants (manifold,
Euler characteristic, volume, normals) are exact statements about index arrays or sign tests; tests/test_marching_tets_cpu.py shows that
the restatement has them, here they are asserted on the GPU's own output.

Lattices: one cell; the smallest interior; small ragged; x across a 32-lane boundary with a ragged scan block; another ragged block; 136
scan blocks of 256 points; 329 scan blocks, so that the single workgroup that scans the block sums loops."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import marching_tets as MT  # noqa: E402
from test_gpu_density import LATTICES, DeviceBuffers  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [(2, 2, 2), (3, 3, 3), (9, 7, 5), (33, 7, 3), (17, 9, 5), (40, 30, 29), (70, 40, 30)]
DIM_IDS = ["x".join(str(d) for d in dims) for dims in DIMS]
RESOLVED = [(40, 30, 29), (70, 40, 30)]      # steps <= 0.071: every feature of the closed fields (smallest radius 0.26) spans several cells
FIELDS = {
    "sphere": lambda lo, step, dims: MT.sphere_field(lo, step, dims),
    "two_spheres": lambda lo, step, dims: MT.two_spheres_field(lo, step, dims),
    "torus": lambda lo, step, dims: MT.torus_field(lo, step, dims),
    "plane": lambda lo, step, dims: MT.plane_field(lo, step, dims),
    "integer": lambda lo, step, dims: MT.integer_field(dims),
}
CLOSED = ("sphere", "two_spheres", "torus")
EULER = {"sphere": 2, "two_spheres": 4, "torus": 0}
NET_LATTICES = [3, 5]                         # of test_gpu_density.LATTICES: 33 x 7 x 3 and 40 x 30 x 29
NETS = ["coarse", "fine"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _assert_same_mesh(got, want_v, want_n, want_t):
    assert got.vertices.shape == want_v.shape and got.triangles.shape == want_t.shape, (got.vertices.shape, want_v.shape, got.triangles.shape, want_t.shape)
    assert got.triangles.dtype == np.uint32 and np.array_equal(got.triangles, want_t), np.flatnonzero((got.triangles != want_t).any(axis=1))[:8]
    bad = np.flatnonzero((_bits(got.vertices) != _bits(want_v)).any(axis=1))
    assert bad.size == 0, (bad[:8], got.vertices[bad[:4]], want_v[bad[:4]])
    if want_n is not None:
        bad = np.flatnonzero((_bits(got.normals) != _bits(want_n)).any(axis=1))
        assert bad.size == 0, (bad[:8], got.normals[bad[:4]], want_n[bad[:4]])


@functools.lru_cache(maxsize=None)
def _case(field, dims):
    """(lo, step, sigma, reference vertices, normals, triangles), computed once and left unchanged."""
    lo, step = MT.unit_lattice(dims)
    sigma = FIELDS[field](lo, step, dims)
    out = (lo, step, sigma) + MT.marching_tets(sigma, lo, step, 0.0)
    for a in out:
        a.setflags(write=False)
    return out


def _border_below(sigma):
    b = np.ones(sigma.shape, bool)
    b[1:-1, 1:-1, 1:-1] = False
    return bool((sigma[b] < 0).all())


# ---- 1. GPU == restatement, bit for bit, on every field and lattice; the invariants on the GPU's own output --------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
@pytest.mark.parametrize("field", list(FIELDS))
def test_gpu_equals_the_restatement(native, renderer, field, dims):
    lo, step, sigma, rv, rn, rt = _case(field, dims)
    got = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True)
    print(f"\n{field} {dims}: {len(got.vertices)} vertices, {len(got.triangles)} triangles")
    _assert_same_mesh(got, rv, rn, rt)
    again = native.isosurface(renderer, sigma, lo, step, 0.0, normals=False, capacity=(len(rv) + 3, len(rt) + 5))   # one call, spare capacity, no normals
    assert again.normals is None
    _assert_same_mesh(again, rv, None, rt)
    t = got.triangles
    if len(t):
        assert (t.min(axis=1) == t[:, 0]).all() and t.max() == len(got.vertices) - 1      # canonical form; every vertex is used
    if field == "integer" and min(dims) > 2:
        assert (sigma == 0).any()                                 # sigma == iso occurs at corners
    if field in CLOSED or (field == "integer" and _border_below(sigma)):
        assert _border_below(sigma)
        if len(t) == 0:
            assert not (sigma > 0).any()                          # a lattice too coarse to catch the field
        else:
            assert MT.is_closed_manifold(t)                       # in index terms: also where sigma == iso makes positions coincide
            assert MT.signed_volume(got.vertices, t) > 0
    if field in EULER and dims in RESOLVED:
        assert MT.euler_characteristic(len(got.vertices), t) == EULER[field]


@pytest.mark.parametrize("dims", DIMS[1:], ids=DIM_IDS[1:])
def test_sphere_vertices_lie_on_their_edges(native, renderer, dims):
    lo, step, sigma, rv, rn, rt = _case("sphere", dims)
    v = native.isosurface(renderer, sigma, lo, step, 0.0).vertices
    a, b = MT.vertex_edges(sigma, 0.0)
    ax = MT.lattice_axes(lo, step, dims)
    pa = np.stack([ax[k][a[:, k]] for k in range(3)], axis=1).astype(np.float64)
    pb = np.stack([ax[k][b[:, k]] for k in range(3)], axis=1).astype(np.float64)
    assert len(v) == len(a) > 0
    r = np.linalg.norm(v.astype(np.float64) - np.array([0.03, -0.02, 0.05]), axis=1)
    slack = 4 * np.finfo(F).eps * 2                               # float32 positions of magnitude <= 1.1 (the field itself is rounded to float32 too)
    assert (np.abs(r - 0.71) <= np.linalg.norm(pb - pa, axis=1) + slack).all()   # the true crossing lies on the same edge


def _analytic_outward(field, c):
    if field == "sphere":
        d = c - np.array([0.03, -0.02, 0.05])
    elif field == "plane":
        return np.tile(np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81]), (len(c), 1))
    else:                                                         # torus: away from the nearest point of the centre circle
        q = c[:, :2] - np.array([0.01, -0.02])
        ring = q / np.linalg.norm(q, axis=1)[:, None] * 0.6
        d = c - np.concatenate([ring + np.array([0.01, -0.02]), np.full((len(c), 1), 0.015)], axis=1)
    return d / np.linalg.norm(d, axis=1)[:, None]


@pytest.mark.parametrize("field", ["sphere", "plane", "torus"])
def test_triangle_normals_point_towards_lower_density(native, renderer, field):
    lo, step, sigma, rv, rn, rt = _case(field, (40, 30, 29))
    got = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True)
    tn, c = MT.triangle_normals_and_centroids(got.vertices, got.triangles)
    dots = np.einsum("ij,ij->i", tn, _analytic_outward(field, c))
    assert len(got.triangles) > 1000 and (dots > 0).all(), (int((dots <= 0).sum()), dots.min())
    vn = np.einsum("ij,ij->i", got.normals.astype(np.float64), _analytic_outward(field, got.vertices.astype(np.float64)))
    assert vn.min() > 0.9                                         # the vertex normals: unit vectors close to -grad sigma / |grad sigma|
    assert np.abs(np.linalg.norm(got.normals.astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- 2. negative steps: the triangle array is the unmirrored one --------------------------------------------------------------------------
@pytest.mark.parametrize("signs", [(-1, 1, 1), (1, -1, -1), (-1, -1, -1)], ids=str)
def test_mirrored_lattice(native, renderer, signs):
    dims = (17, 9, 5)
    lo, step, sigma, rv, rn, rt = _case("sphere", dims)
    hi = (lo + step * (F(dims) - 1)).astype(F)
    lo2 = F([hi[k] if signs[k] < 0 else lo[k] for k in range(3)]); step2 = (step * F(signs)).astype(F)
    got = native.isosurface(renderer, sigma, lo2, step2, 0.0, normals=True)
    assert np.array_equal(got.triangles, rt) and len(rt) > 0     # winding lives in index space
    mv, mn, mt = MT.marching_tets(sigma, lo2, step2, 0.0)
    _assert_same_mesh(got, mv, mn, mt)
    vol = MT.signed_volume(got.vertices, got.triangles)
    assert (vol < 0) == (np.prod(signs) < 0) and vol != 0         # an odd number of negative steps: wound inwards in world space


# ---- 3. nothing to extract; non-finite sigma ---------------------------------------------------------------------------------------------------
def test_all_below_and_all_above(native, renderer):
    for dims in ((2, 2, 2), (33, 7, 3)):
        lo, step = MT.unit_lattice(dims)
        for value in (-1.0, 1.0, 0.0):                             # sigma == iso everywhere: nothing is inside
            m = native.isosurface(renderer, np.full(dims[::-1], value, F), lo, step, 0.0, normals=True)
            assert m.vertices.shape == (0, 3) and m.normals.shape == (0, 3) and m.triangles.shape == (0, 3)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_cells_around_a_non_finite_sigma_are_skipped(native, renderer, bad):
    dims = (17, 9, 5)
    lo, step, sigma, rv, rn, rt = _case("sphere", dims)
    a, b = MT.vertex_edges(sigma, 0.0)
    s = sigma.copy()
    ix, iy, iz = a[len(a) // 2]                                   # a lattice point that owns a vertex: the surface passes through its cells
    s[iz, iy, ix] = bad
    s[0, 0, 0] = bad                                              # and a corner of the lattice
    got = native.isosurface(renderer, s, lo, step, 0.0, normals=True)
    wv, wn, wt = MT.marching_tets(s, lo, step, 0.0)
    assert 0 < len(wt) < len(rt) and len(wv) < len(rv)
    assert got.vertices.shape == wv.shape and got.triangles.shape == wt.shape and np.array_equal(got.triangles, wt)
    assert _same_bits(got.vertices, wv) and np.isfinite(got.vertices).all()
    # normals next to the hole take the non-finite sigma into a central difference: zero vectors there, bit-equal everywhere
    assert np.array_equal(_bits(got.normals), _bits(wn)) and np.isfinite(got.normals).all() and (np.abs(got.normals).sum(axis=1) == 0).any()
    assert not MT.is_closed_manifold(got.triangles)               # the skipped cells leave a hole


# ---- 4. the capacity protocol, through the C ABI ---------------------------------------------------------------------------------------------
def _raw_grid(native, renderer, sigma, lo, step, iso, v, n, cap_v, t, cap_t):
    from nerf_rs_amd import _lib
    L = native.load_library()
    dims = np.int32(sigma.shape[::-1]); lo = F(lo); step = F(step)
    nv, nt = C.c_uint64(12345), C.c_uint64(54321)
    p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
    rc = L.nerf_isosurface_grid(renderer.handle, p(sigma, _lib.f32p), p(lo, _lib.f32p), p(step, _lib.f32p), p(dims, _lib.i32p), iso, p(v, _lib.f32p),
                                p(n, _lib.f32p), cap_v, p(t, _lib.u32p), cap_t, C.byref(nv), C.byref(nt))
    return rc, int(nv.value), int(nt.value)


def test_capacity_protocol(native, renderer):
    lo, step, sigma, rv, rn, rt = _case("torus", (17, 9, 5))
    V, T = len(rv), len(rt)
    assert _raw_grid(native, renderer, sigma, lo, step, 0.0, None, None, 0, None, 0) == (0, V, T)           # the size query
    for cap_v, cap_t in ((V - 1, T), (V, T - 1), (0, 0), (V - 1, T - 1)):
        v, n, t = np.full((V + 1, 3), -7.5, F), np.full((V + 1, 3), -7.5, F), np.full((T + 1, 3), 0xDEADBEEF, np.uint32)
        assert _raw_grid(native, renderer, sigma, lo, step, 0.0, v, n, cap_v, t, cap_t) == (0, V, T)        # NERF_OK, counts returned ...
        assert (v == F(-7.5)).all() and (n == F(-7.5)).all() and (t == 0xDEADBEEF).all()                    # ... nothing written
    v, n, t = np.full((V + 1, 3), -7.5, F), np.full((V + 1, 3), -7.5, F), np.full((T + 1, 3), 0xDEADBEEF, np.uint32)
    assert _raw_grid(native, renderer, sigma, lo, step, 0.0, v, n, V, t, T) == (0, V, T)                    # exact capacities: filled, nothing beyond
    assert _same_bits(v[:V], rv) and _same_bits(n[:V], rn) and np.array_equal(t[:T], rt)
    assert (v[V] == F(-7.5)).all() and (n[V] == F(-7.5)).all() and (t[T] == 0xDEADBEEF).all()
    t = np.full((T, 3), 0xDEADBEEF, np.uint32)                                                              # any subset of the arrays
    assert _raw_grid(native, renderer, sigma, lo, step, 0.0, None, None, V, t, T) == (0, V, T) and np.array_equal(t, rt)
    with pytest.raises(native.NerfError) as e:
        native.isosurface(renderer, sigma, lo, step, 0.0, capacity=(V - 1, T))
    assert e.value.code == -1 and str(V) in e.value.msg


def test_argument_errors_with_a_live_context(native, renderer):
    lo, step, sigma, rv, rn, rt = _case("sphere", (3, 3, 3))
    inf = float("inf")
    for kw in (dict(lo=(0, inf, 0)), dict(step=(0.1, 0.0, 0.1)), dict(step=(0.1, float("nan"), 0.1)), dict(iso=inf), dict(iso=float("nan"))):
        args = dict(lo=lo, step=step, iso=0.0); args.update(kw)
        with pytest.raises(native.NerfError) as e:
            native.isosurface(renderer, sigma, **args)
        assert e.value.code == -1, (kw, e.value)
    with pytest.raises(native.NerfError) as e:
        native.isosurface(renderer, np.zeros((2, 1, 2), F), lo, step, 0.0)
    assert e.value.code == -1
    for dims in ((1, 2, 2), (65536, 65536, 2), (1024, 1024, 257)):
        with pytest.raises(native.NerfError) as e:
            renderer.fine.extract_mesh(lo, step, dims, 1.0)
        assert e.value.code == -1, dims


def test_no_network_is_needed_for_a_caller_lattice(native):
    lo, step, sigma, rv, rn, rt = _case("two_spheres", (9, 7, 5))
    with native.Renderer(0) as r:
        _assert_same_mesh(native.isosurface(r, sigma, lo, step, 0.0, normals=True), rv, rn, rt)
        net = native.Network(r, 1)
        with pytest.raises(native.NerfError) as e:
            net.extract_mesh((0, 0, 0), (0.1, 0.1, 0.1), (3, 3, 3), 1.0)
        assert e.value.code == -6 and "not loaded" in e.value.msg
        with pytest.raises(native.NerfError) as e:                # argument errors come first
            net.extract_mesh((0, 0, 0), (0.1, 0.1, 0.1), (3, 1, 3), 1.0)
        assert e.value.code == -1


# ---- 5. the network entry points ------------------------------------------------------------------------------------------------------------
def _net(renderer, name):
    return renderer.coarse if name == "coarse" else renderer.fine


@pytest.fixture(scope="module")
def net_cases(renderer):
    """(lattice, network) -> (sigma grid of nerf_density_grid, iso = the median of its positive values), computed once."""
    out = {}
    for k in NET_LATTICES:
        lo, step, dims = LATTICES[k]
        for name in NETS:
            sig = _net(renderer, name).density_grid(lo, step, dims)[0]
            assert (sig > 0).any() and (sig == 0).any()
            iso = float(np.median(sig[sig > 0]))
            sig.setflags(write=False)
            out[k, name] = (sig, iso)
    return out


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("k", NET_LATTICES)
def test_extract_mesh_equals_isosurface_of_the_density_grid(native, renderer, net_cases, k, name):
    lo, step, dims = LATTICES[k]
    sig, iso = net_cases[k, name]
    net = _net(renderer, name)
    want = native.isosurface(renderer, sig, lo, step, iso, normals=True)
    got = net.extract_mesh(lo, step, dims, iso, normals=True, colours=True)
    print(f"\n{dims} {name}: iso {iso:.4g}, {len(got.vertices)} vertices, {len(got.triangles)} triangles")
    assert len(got.triangles) > 0
    _assert_same_mesh(got, want.vertices, want.normals, want.triangles)
    rv, rn, rt = MT.marching_tets(sig, lo, step, iso)             # and the restatement on the network's field
    _assert_same_mesh(got, rv, rn, rt)
    # colours: forward_batch at the vertices, looking at the surface head-on
    rgb, _ = net.forward_batch(np.ascontiguousarray(got.vertices.T), -got.normals)
    assert got.colours.shape == rgb.shape and np.array_equal(_bits(got.colours), _bits(rgb))
    assert np.ptp(got.colours, axis=0).max() > 0.05 and np.isfinite(got.colours).all()
    plain = net.extract_mesh(lo, step, dims, iso, capacity=(len(got.vertices), len(got.triangles)))   # no normals, no colours: the same mesh
    assert plain.normals is None and plain.colours is None
    _assert_same_mesh(plain, want.vertices, None, want.triangles)


def test_extract_mesh_device_entry_point(native, renderer, net_cases):
    k, name = 3, "fine"
    lo, step, dims = LATTICES[k]
    sig, iso = net_cases[k, name]
    want = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True)
    V, T = len(want.vertices), len(want.triangles)
    d = DeviceBuffers(native)
    try:
        assert renderer.fine.extract_mesh_device(lo, step, dims, iso, None, None, None, 0, None, 0) == (V, T)
        d_v, d_n, d_c = (d.upload(np.full((V + 1, 3), -7.5, F)) for _ in range(3))
        d_t = d.upload(np.full((T + 1, 3), 0xDEADBEEF, np.uint32))
        assert renderer.fine.extract_mesh_device(lo, step, dims, iso, d_v, d_n, d_c, V - 1, d_t, T) == (V, T)    # one short: untouched
        assert (d.download(d_v, (V + 1, 3), F) == F(-7.5)).all() and (d.download(d_t, (T + 1, 3), np.uint32) == 0xDEADBEEF).all()
        assert renderer.fine.extract_mesh_device(lo, step, dims, iso, d_v, d_n, d_c, V + 1, d_t, T + 1) == (V, T)
        v, n, c, t = d.download(d_v, (V + 1, 3), F), d.download(d_n, (V + 1, 3), F), d.download(d_c, (V + 1, 3), F), d.download(d_t, (T + 1, 3), np.uint32)
        assert _same_bits(v[:V], want.vertices) and _same_bits(n[:V], want.normals) and _same_bits(c[:V], want.colours) and np.array_equal(t[:T], want.triangles)
        assert (v[V] == F(-7.5)).all() and (n[V] == F(-7.5)).all() and (c[V] == F(-7.5)).all() and (t[T] == 0xDEADBEEF).all()
    finally:
        d.close()


def test_cli_writes_the_library_mesh(native, renderer, net_cases, tmp_path):
    k, name = 3, "coarse"
    lo, step, dims = LATTICES[k]
    sig, iso = net_cases[k, name]
    exe = os.path.join(ROOT, "nerf-rs_amd", "nerf_cli")
    exact = lambda v: ",".join(repr(float(F(x))) for x in v)
    grid = ["--scene", SCENE, "--density-grid", ",".join(str(d) for d in dims), "--grid-lo", exact(lo), "--grid-step", exact(step), "--grid-net", name]
    res = subprocess.run([exe] + grid + ["--mesh", str(tmp_path / "m.ply"), "--mesh-iso", repr(float(F(iso))), "--mesh-colour"],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    m = renderer.coarse.extract_mesh(lo, step, dims, iso, normals=True, colours=True)
    native.save_ply(tmp_path / "want.ply", m.vertices, m.triangles, normals=m.normals, colours=m.colours)
    assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    assert f"{len(m.vertices)} vertices, {len(m.triangles)} triangles" in res.stdout
    assert "Rendering" not in res.stdout and not (tmp_path / "output.ppm").exists()      # only a mesh was asked for: no render
    res = subprocess.run([exe] + grid + ["--mesh", str(tmp_path / "n.ply"), "--mesh-iso", repr(float(F(iso)))], capture_output=True, text=True, timeout=120,
                         cwd=str(tmp_path))
    native.save_ply(tmp_path / "want2.ply", m.vertices, m.triangles, normals=m.normals)
    assert res.returncode == 0 and (tmp_path / "n.ply").read_bytes() == (tmp_path / "want2.ply").read_bytes()
    assert subprocess.run([exe, "--scene", SCENE, "--mesh", "x.ply"], capture_output=True, cwd=str(tmp_path)).returncode == 2      # no lattice
    assert subprocess.run([exe] + grid + ["--mesh-iso", "3"], capture_output=True, cwd=str(tmp_path)).returncode == 2               # no --mesh


def test_render_is_unchanged_by_a_mesh_call(native, renderer, samples, net_cases):
    cam = native.camera_from_samples(samples, 256, 256, 32)
    crop = (96, 104, 64, 48)
    before = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    lo, step, dims = LATTICES[5]
    m = renderer.fine.extract_mesh(lo, step, dims, net_cases[5, "fine"][1], normals=True, colours=True)
    again = renderer.fine.extract_mesh(lo, step, dims, net_cases[5, "fine"][1], normals=True, colours=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(m, again))      # deterministic: the same bits in every run
    after = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    assert before.shape == (48, 64, 3) and _same_bits(after, before)
