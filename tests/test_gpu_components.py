"""Lattice components and filtered meshes on the GPU: nerf_lattice_components (labels, sizes, rank order, bounds) and the *_filtered mesh entry
points against the restatement tests/helpers/lattice_components.py (flood fill; tests/test_lattice_components_cpu.py shows it fit for purpose).

Stated tolerances: none.  Labels, counts, sizes and bounds are integers fixed by the definition in the header; the filtered mesh is the
unfiltered mesh of tests/helpers/marching_tets.py minus the discarded components' vertices and triangles with ids renumbered in order, so
vertices, normals and triangles must agree BIT FOR BIT.

Lattices: a single point; one cell; the smallest interior; small ragged; x across a wave boundary; 136 blocks of 256 points; 329 blocks, so that
labels, the root compaction and the ranking cross many workgroups."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lattice_components as LC  # noqa: E402
import marching_tets as MT  # noqa: E402
from test_gpu_density import LATTICES, DeviceBuffers  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (9, 7, 5), (33, 7, 3), (40, 30, 29), (70, 40, 30)]
DIM_IDS = ["x".join(str(d) for d in dims) for dims in DIMS]


def _planted(dims):
    s = LC.noise(dims, 0.3, 5).copy()
    flat = s.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf)):
        flat[(k * 7919 + 3) % flat.size] = v
    flat[flat.size - 1] = np.inf
    return s


FIELDS = {
    "floaters": LC.floaters,
    "snake": LC.snake,
    "hollow": LC.hollow,
    "noise12": lambda dims: LC.noise(dims, 0.12, 1),
    "noise20": lambda dims: LC.noise(dims, 0.2, 2),
    "all_inside": lambda dims: np.ones(dims[::-1], F),
    "all_outside": lambda dims: np.zeros(dims[::-1], F),
    "planted": _planted,
}


@functools.lru_cache(maxsize=None)
def _case(field, dims):
    """(sigma, reference labels, reference table), computed once and left unchanged."""
    sigma = np.ascontiguousarray(FIELDS[field](dims), F)
    labels, table = LC.components(sigma, 0.0)
    sigma.setflags(write=False); labels.setflags(write=False)
    return sigma, labels, table


def _as_tuples(components):
    return [(c.label, c.n_points, tuple(c.bounds)) for c in components]


# ---- 1. labels, tables, counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=DIM_IDS)
@pytest.mark.parametrize("field", list(FIELDS))
def test_labels_table_and_count_equal_the_restatement(native, renderer, field, dims):
    sigma, want_labels, want_table = _case(field, dims)
    labels, comps, n = native.lattice_components(renderer, sigma, 0.0, table=64)
    print(f"\n{field} {dims}: {n} components, largest {[c.n_points for c in comps[:4]]}")
    assert n == len(want_table)
    assert labels.dtype == np.uint32 and labels.shape == sigma.shape
    bad = np.flatnonzero(labels.reshape(-1) != want_labels.reshape(-1))
    assert bad.size == 0, (bad[:8], labels.reshape(-1)[bad[:8]], want_labels.reshape(-1)[bad[:8]])
    assert _as_tuples(comps) == want_table[:64]
    none, comps1, n1 = native.lattice_components(renderer, sigma, 0.0, table=1, want_labels=False)
    assert none is None and n1 == n and _as_tuples(comps1) == want_table[:1]


def _raw_components(native, renderer, sigma, iso, labels, table, cap):
    L = native.load_library()
    dims = np.int32(sigma.shape[::-1])
    n = C.c_uint64(0xABCDEF)
    from nerf_rs_amd import _lib
    rc = L.nerf_lattice_components(renderer.handle, sigma.ctypes.data_as(_lib.f32p), dims.ctypes.data_as(_lib.i32p), iso,
                                   None if labels is None else labels.ctypes.data_as(_lib.u32p), None if table is None else table.ctypes.data, cap, C.byref(n))
    return rc, int(n.value)


@pytest.mark.parametrize("field,dims", [("floaters", (40, 30, 29)), ("noise12", (70, 40, 30)), ("all_outside", (9, 7, 5))], ids=str)
def test_table_capacities_write_nothing_beyond_the_count(native, renderer, field, dims):
    sigma, want_labels, want_table = _case(field, dims)
    n_comp = len(want_table)
    for cap in (0, 1, 64):
        table = np.full((65, 8), 0xDEADBEEF, np.uint32)              # 8 words per nerf_component, one spare entry
        rc, n = _raw_components(native, renderer, sigma, 0.0, None, table if cap else None, cap)
        assert (rc, n) == (0, n_comp)
        filled = min(cap, n_comp)
        got = [(int(r[0]), int(r[1]), tuple(int(v) for v in r[2:].view(np.int32))) for r in table[:filled]]
        assert got == want_table[:filled]
        assert (table[filled:] == 0xDEADBEEF).all()                  # cap larger than the number of components: the rest is untouched
    with pytest.raises(native.NerfError) as e:
        native.lattice_components(renderer, sigma, 0.0, table=65)
    assert e.value.code == -1


def test_other_iso_values(native, renderer):
    sigma, _, _ = _case("noise20", (40, 30, 29))
    for iso in (-0.5, 0.45, 2.0):
        want_labels, want_table = LC.components(sigma, iso)
        labels, comps, n = native.lattice_components(renderer, sigma, iso, table=8)
        assert n == len(want_table) and np.array_equal(labels, want_labels) and _as_tuples(comps) == want_table[:8]


# ---- 2. filtered meshes --------------------------------------------------------------------------------------------------------------------------
MESH_DIMS = (40, 30, 29)
MESH_FIELDS = {
    "floaters": LC.floaters,
    "two_spheres": lambda dims: MT.two_spheres_field(*MT.unit_lattice(dims), dims),
    "hollow": LC.hollow,
    "noise20": lambda dims: LC.noise(dims, 0.2, 2),
    "noise12": lambda dims: LC.noise(dims, 0.12, 1),
}


@functools.lru_cache(maxsize=None)
def _mesh_case(field):
    lo, step = MT.unit_lattice(MESH_DIMS)
    sigma = np.ascontiguousarray(MESH_FIELDS[field](MESH_DIMS), F)
    out = (lo, step, sigma) + MT.marching_tets(sigma, lo, step, 0.0) + (LC.components(sigma, 0.0),)
    for a in out[:-1]:
        a.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _assert_same_mesh(got, want_v, want_n, want_t):
    assert got.vertices.shape == want_v.shape and got.triangles.shape == want_t.shape, (got.vertices.shape, want_v.shape, got.triangles.shape, want_t.shape)
    assert got.triangles.dtype == np.uint32 and np.array_equal(got.triangles, want_t)
    assert np.array_equal(_bits(got.vertices), _bits(want_v))
    if want_n is not None:
        assert np.array_equal(_bits(got.normals), _bits(want_n))


def _filters(table):
    sizes = [e[1] for e in table]
    between = (sizes[1] + sizes[2] + 1) // 2 if len(sizes) > 2 and sizes[1] > sizes[2] else max(sizes[min(1, len(sizes) - 1)], 2)
    return [(1, 0), (3, 0), (0, between), (2, between), (0, 0), (0, 1), (64, 0), (5, 10 ** 7), (0, 2 ** 32 - 1)]


@pytest.mark.parametrize("field", list(MESH_FIELDS))
def test_filtered_mesh_equals_the_filtered_restatement(native, renderer, field):
    lo, step, sigma, rv, rn, rt, labelled = _mesh_case(field)
    for keep_largest, min_points in _filters(labelled[1]):
        wv, wn, wt, n_comp, n_kept = LC.filter_mesh(sigma, 0.0, rv, rn, rt, keep_largest, min_points, labelled=labelled)
        got, gc, gk = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True, keep_largest=keep_largest, min_points=min_points, return_counts=True)
        print(f"\n{field} keep_largest={keep_largest} min_points={min_points}: {gk} of {gc} components, {len(got.vertices)} of {len(rv)} vertices, "
              f"{len(got.triangles)} of {len(rt)} triangles")
        assert (gc, gk) == (n_comp, n_kept), (keep_largest, min_points)
        _assert_same_mesh(got, wv, wn, wt)
        if min_points > 10 ** 6:
            assert (len(got.vertices), len(got.triangles), gk) == (0, 0, 0)      # a filter that keeps nothing
    plain = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True)      # the unfiltered entry point ...
    _assert_same_mesh(plain, rv, rn, rt)
    null = _raw_filtered(native, renderer, sigma, lo, step, None, len(rv), len(rt), counts=False)     # ... equals a NULL filter, bit for bit
    assert null[:3] == (0, len(rv), len(rt)) and np.array_equal(_bits(null[3]), _bits(plain.vertices)) and np.array_equal(_bits(null[4]), _bits(plain.normals))
    assert np.array_equal(null[5], plain.triangles)
    zero = _raw_filtered(native, renderer, sigma, lo, step, (0, 0), len(rv), len(rt))                # ... and a non-NULL {0, 0} filter, with both counts
    assert zero[:3] == (0, len(rv), len(rt)) and zero[6:8] == (len(labelled[1]), len(labelled[1]))
    assert np.array_equal(_bits(zero[3]), _bits(plain.vertices)) and np.array_equal(_bits(zero[4]), _bits(plain.normals)) and np.array_equal(zero[5], plain.triangles)


def _raw_filtered(native, renderer, sigma, lo, step, filt, cap_v, cap_t, counts=True, arrays=True):
    """nerf_isosurface_grid_filtered with sentinel-filled arrays one entry larger than the capacities -> (rc, nv, nt, v, n, t, n_components, n_kept)."""
    from nerf_rs_amd import _lib
    L = native.load_library()
    dims = np.int32(sigma.shape[::-1]); lo = F(lo); step = F(step)
    v, n, t = np.full((cap_v + 1, 3), -7.5, F), np.full((cap_v + 1, 3), -7.5, F), np.full((cap_t + 1, 3), 0xDEADBEEF, np.uint32)
    nv, nt, nc, nk = C.c_uint64(1), C.c_uint64(2), C.c_uint64(3), C.c_uint64(4)
    f = None if filt is None else _lib.CComponentFilter(*filt)
    rc = L.nerf_isosurface_grid_filtered(renderer.handle, sigma.ctypes.data_as(_lib.f32p), lo.ctypes.data_as(_lib.f32p), step.ctypes.data_as(_lib.f32p),
                                         dims.ctypes.data_as(_lib.i32p), 0.0, None if f is None else C.addressof(f),
                                         v.ctypes.data_as(_lib.f32p) if arrays else None, n.ctypes.data_as(_lib.f32p) if arrays else None, cap_v if arrays else 0,
                                         t.ctypes.data_as(_lib.u32p) if arrays else None, cap_t if arrays else 0, C.byref(nv), C.byref(nt),
                                         C.byref(nc) if counts else None, C.byref(nk) if counts else None)
    return rc, int(nv.value), int(nt.value), v[:cap_v], n[:cap_v], t[:cap_t], int(nc.value), int(nk.value), v[cap_v], t[cap_t]


def test_capacity_protocol_with_filtered_counts(native, renderer):
    lo, step, sigma, rv, rn, rt, labelled = _mesh_case("floaters")
    wv, wn, wt, n_comp, n_kept = LC.filter_mesh(sigma, 0.0, rv, rn, rt, 2, 0, labelled=labelled)
    V, T = len(wv), len(wt)
    assert 0 < V < len(rv) and 0 < T < len(rt)
    r = _raw_filtered(native, renderer, sigma, lo, step, (2, 0), 0, 0, arrays=False)                # the size query returns the FILTERED counts
    assert (r[0], r[1], r[2], r[6], r[7]) == (0, V, T, n_comp, 2)
    for cap_v, cap_t in ((V - 1, T), (V, T - 1)):
        r = _raw_filtered(native, renderer, sigma, lo, step, (2, 0), cap_v, cap_t)
        assert (r[0], r[1], r[2]) == (0, V, T) and (r[3] == F(-7.5)).all() and (r[5] == 0xDEADBEEF).all()      # counts returned, nothing written
    r = _raw_filtered(native, renderer, sigma, lo, step, (2, 0), V, T)                              # the filtered counts fit: filled, nothing beyond
    assert (r[0], r[1], r[2]) == (0, V, T)
    assert np.array_equal(_bits(r[3]), _bits(wv)) and np.array_equal(_bits(r[4]), _bits(wn)) and np.array_equal(r[5], wt)
    assert (r[8] == F(-7.5)).all() and (r[9] == 0xDEADBEEF).all()
    with pytest.raises(native.NerfError) as e:
        native.isosurface(renderer, sigma, lo, step, 0.0, capacity=(V - 1, T), keep_largest=2)
    assert e.value.code == -1 and str(V) in e.value.msg
    with pytest.raises(native.NerfError) as e:
        native.isosurface(renderer, sigma, lo, step, 0.0, keep_largest=65)
    assert e.value.code == -1 and "keep_largest" in e.value.msg


# ---- 3. the lego networks ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lego(renderer):
    """The 40 x 30 x 29 lattice of test_gpu_density: (lo, step, dims, sigma of the fine network, iso = the median positive sigma)."""
    lo, step, dims = LATTICES[5]
    sig = renderer.fine.density_grid(lo, step, dims)[0]
    iso = float(np.median(sig[sig > 0]))
    sig.setflags(write=False)
    return lo, step, dims, sig, iso


def test_extract_mesh_keep_largest_equals_isosurface_of_the_density_grid(native, renderer, lego):
    lo, step, dims, sig, iso = lego
    want, wc, wk = native.isosurface(renderer, sig, lo, step, iso, normals=True, keep_largest=1, return_counts=True)
    got, gc, gk = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True, keep_largest=1, return_counts=True)
    full = renderer.fine.extract_mesh(lo, step, dims, iso)
    print(f"\nlego {dims} iso {iso:.4g}: {gc} components, largest keeps {len(got.vertices)} of {len(full.vertices)} vertices")
    assert (gc, gk) == (wc, wk) and gk == 1 and gc > 1 and 0 < len(got.triangles) < len(full.triangles)
    _assert_same_mesh(got, want.vertices, want.normals, want.triangles)
    rv, rn, rt = MT.marching_tets(sig, lo, step, iso)                 # and the restatement on the network's field
    wv, wn, wt, n_comp, n_kept = LC.filter_mesh(sig, iso, rv, rn, rt, 1, 0)
    assert (gc, gk) == (n_comp, n_kept)
    _assert_same_mesh(got, wv, wn, wt)
    rgb, _ = renderer.fine.forward_batch(np.ascontiguousarray(got.vertices.T), -got.normals)
    assert np.array_equal(_bits(got.colours), _bits(rgb))             # colours: forward_batch at the kept vertices
    labels, comps, n = native.lattice_components(renderer, sig, iso, table=4)
    assert n == gc and comps[0].n_points == LC.components(sig, iso)[1][0][1]


def test_device_entry_points_equal_the_host_ones(native, renderer, lego):
    lo, step, dims, sig, iso = lego
    want = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True, keep_largest=1)
    V, T = len(want.vertices), len(want.triangles)
    want_labels, want_comps, want_n = native.lattice_components(renderer, sig, iso, table=16)
    d = DeviceBuffers(native)
    try:
        d_v, d_n, d_c = (d.upload(np.full((V + 1, 3), -7.5, F)) for _ in range(3))
        d_t = d.upload(np.full((T + 1, 3), 0xDEADBEEF, np.uint32))
        out = renderer.fine.extract_mesh_device(lo, step, dims, iso, d_v, d_n, d_c, V + 1, d_t, T + 1, keep_largest=1, return_counts=True)
        assert out == (V, T, want_n, 1)
        v, n, c, t = d.download(d_v, (V + 1, 3), F), d.download(d_n, (V + 1, 3), F), d.download(d_c, (V + 1, 3), F), d.download(d_t, (T + 1, 3), np.uint32)
        assert np.array_equal(_bits(v[:V]), _bits(want.vertices)) and np.array_equal(_bits(n[:V]), _bits(want.normals))
        assert np.array_equal(_bits(c[:V]), _bits(want.colours)) and np.array_equal(t[:T], want.triangles)
        assert (v[V] == F(-7.5)).all() and (t[T] == 0xDEADBEEF).all()
        # sigma never reaches the host: density_grid_device -> lattice_components_device
        N = int(np.prod(dims))
        d_sigma = d.upload(np.zeros(N, F)); d_labels = d.upload(np.full(N + 1, 0x5A5A5A5A, np.uint32))
        renderer.fine.density_grid_device(lo, step, dims, d_sigma=d_sigma)
        comps, n = native.lattice_components_device(renderer, d_sigma, dims, iso, d_labels=d_labels, table=16)
        assert n == want_n and comps == want_comps
        labels = d.download(d_labels, (N + 1,), np.uint32)
        assert np.array_equal(labels[:N].reshape(want_labels.shape), want_labels) and labels[N] == 0x5A5A5A5A
    finally:
        d.close()


def test_cli_writes_the_largest_component(native, renderer, lego, tmp_path):
    lo, step, dims, sig, iso = lego
    exe = os.path.join(ROOT, "nerf-rs_amd", "nerf_cli")
    exact = lambda v: ",".join(repr(float(F(x))) for x in v)
    grid = ["--scene", SCENE, "--density-grid", ",".join(str(d) for d in dims), "--grid-lo", exact(lo), "--grid-step", exact(step), "--grid-net", "fine"]
    res = subprocess.run([exe] + grid + ["--mesh", str(tmp_path / "m.ply"), "--mesh-iso", repr(float(F(iso))), "--mesh-colour", "--mesh-keep-largest", "1"],
                         capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    m, n_comp, n_kept = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True, keep_largest=1, return_counts=True)
    native.save_ply(tmp_path / "want.ply", m.vertices, m.triangles, normals=m.normals, colours=m.colours)
    assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    assert f"{len(m.vertices)} vertices, {len(m.triangles)} triangles" in res.stdout
    assert f"{n_comp} components, {n_kept} kept" in res.stdout
    assert subprocess.run([exe] + grid + ["--mesh-keep-largest", "1"], capture_output=True, cwd=str(tmp_path)).returncode == 2       # no --mesh


def test_unfiltered_calls_and_renders_are_unchanged_by_a_filtered_call(native, renderer, samples, lego):
    lo, step, dims, sig, iso = lego
    cam = native.camera_from_samples(samples, 256, 256, 32)
    crop = (96, 104, 64, 48)
    before_img = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    before = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True)
    first = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True, keep_largest=1, min_points=3)
    native.lattice_components(renderer, sig, iso, table=64)
    again = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True, keep_largest=1, min_points=3)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, again))      # deterministic: the same bits in every run
    after = renderer.fine.extract_mesh(lo, step, dims, iso, normals=True, colours=True)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, after))     # the workspaces do not alias
    after_img = native.render_image(renderer.coarse, renderer.fine, cam, 64, seed=3, crop=crop)
    assert before_img.shape == (48, 64, 3) and np.array_equal(_bits(after_img), _bits(before_img))


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_returns_the_same_arrays(native, renderer):
    sigma, _, _ = _case("noise20", (70, 40, 30))
    a = native.lattice_components(renderer, sigma, 0.0, table=64)
    b = native.lattice_components(renderer, sigma, 0.0, table=64)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    lo, step = MT.unit_lattice((70, 40, 30))
    m1 = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True, keep_largest=3, min_points=2)
    m2 = native.isosurface(renderer, sigma, lo, step, 0.0, normals=True, keep_largest=3, min_points=2)
    assert len(m1.triangles) > 0 and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip((m1.vertices, m1.normals, m1.triangles), (m2.vertices, m2.normals, m2.triangles)))
