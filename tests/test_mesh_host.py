"""Isosurface meshes, host side (no device): the four entry points exist with the ctypes signatures; every argument error the header lists is
refused before anything touches a context or a device (so a NULL context reaches them, and "ctx is NULL" is the last refusal); the PLY
writer round-trips through a parser written here, with and without normals and colours and with no triangles; and the stand-alone
AddressSanitizer + UBSan driver (`make host-asan`, no HIP, nothing preloaded) runs the writer clean."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MESH_FUNCTIONS = ("nerf_isosurface_grid", "nerf_extract_mesh", "nerf_extract_mesh_device", "nerf_save_ply")
INVALID = -1
F = np.float32


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    f32p, u32p, i32p, u64p, vp, sz = _lib.f32p, _lib.u32p, _lib.i32p, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t
    want = {
        "nerf_isosurface_grid": [vp, f32p, f32p, f32p, i32p, C.c_float, f32p, f32p, sz, u32p, sz, u64p, u64p],
        "nerf_extract_mesh": [vp, C.c_int, f32p, f32p, i32p, C.c_float, f32p, f32p, f32p, sz, u32p, sz, u64p, u64p],
        "nerf_extract_mesh_device": [vp, C.c_int, f32p, f32p, i32p, C.c_float, vp, vp, vp, sz, vp, sz, u64p, u64p, vp],
        "nerf_save_ply": [C.c_char_p, sz, f32p, f32p, f32p, sz, u32p],
    }
    for name in MESH_FUNCTIONS:
        fn = getattr(L, name)                                    # AttributeError without the feature
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args == want[name], name
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    assert L.nerf_abi_version() == 5                              # additive
    for name in ("extract_mesh", "extract_mesh_device"):
        assert callable(getattr(native.Network, name)), name
    assert callable(native.isosurface) and callable(native.save_ply) and native.Mesh._fields == ("vertices", "normals", "colours", "triangles")
    assert "twice" in native.Network.extract_mesh.__doc__.lower()  # a query followed by a fill evaluates the lattice twice: said where the user reads it


def _call(L, entry, ctx=None, which=1, sigma=True, lo=(0.0, 0.0, 0.0), step=(0.1, 0.1, 0.1), dims=(3, 3, 3), iso=1.0, counts=(True, True)):
    """One call with real (small) host buffers; returns (rc, message)."""
    from nerf_rs_amd import _lib
    sig = np.zeros(64, F); v = np.zeros((8, 3), F); n = np.zeros((8, 3), F); c = np.zeros((8, 3), F); t = np.zeros((8, 3), np.uint32)
    nv, nt = C.c_uint64(), C.c_uint64()
    f3 = lambda a: None if a is None else C.cast((C.c_float * 3)(*a), _lib.f32p)
    i3 = None if dims is None else C.cast((C.c_int32 * 3)(*dims), _lib.i32p)
    pv, pt = (C.byref(nv) if counts[0] else None), (C.byref(nt) if counts[1] else None)
    if entry == "grid":
        rc = L.nerf_isosurface_grid(ctx, sig.ctypes.data_as(_lib.f32p) if sigma else None, f3(lo), f3(step), i3, iso, v.ctypes.data_as(_lib.f32p),
                                    n.ctypes.data_as(_lib.f32p), 8, t.ctypes.data_as(_lib.u32p), 8, pv, pt)
    elif entry == "net":
        rc = L.nerf_extract_mesh(ctx, which, f3(lo), f3(step), i3, iso, v.ctypes.data_as(_lib.f32p), n.ctypes.data_as(_lib.f32p), c.ctypes.data_as(_lib.f32p), 8,
                                 t.ctypes.data_as(_lib.u32p), 8, pv, pt)
    else:
        rc = L.nerf_extract_mesh_device(ctx, which, f3(lo), f3(step), i3, iso, v.ctypes.data, n.ctypes.data, c.ctypes.data, 8, t.ctypes.data, 8, pv, pt, None)
    return rc, L.nerf_last_error(None).decode()


@pytest.mark.parametrize("entry", ["grid", "net", "device"])
def test_argument_errors_need_no_device(native, entry):
    L = native.load_library()
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(dims=(1, 3, 3)), "at least 2"), (dict(dims=(3, 0, 3)), "at least 2"), (dict(dims=(3, 3, -4)), "at least 2"), (dict(dims=(1, 1, 1)), "at least 2"),
        (dict(dims=None), "must not be NULL"), (dict(lo=None), "must not be NULL"), (dict(step=None), "must not be NULL"),
        (dict(step=(0.1, 0.0, 0.1)), "step must not be 0"), (dict(step=(-0.0, 0.1, 0.1)), "step must not be 0"),
        (dict(lo=(0.0, nan, 0.0)), "finite"), (dict(lo=(inf, 0.0, 0.0)), "finite"), (dict(step=(0.1, 0.1, -inf)), "finite"), (dict(step=(nan, 0.1, 0.1)), "finite"),
        (dict(iso=nan), "finite"), (dict(iso=inf), "finite"), (dict(iso=-inf), "finite"),
        (dict(dims=(1024, 1024, 257)), "too large"),                # one plane beyond 2^28
        (dict(dims=(65536, 65536, 2)), "too large"), (dict(dims=(2 ** 31 - 1, 2, 2)), "too large"), (dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "too large"),
        (dict(counts=(False, True)), "required"), (dict(counts=(True, False)), "required"),
    ]
    if entry == "grid":
        cases += [(dict(sigma=False), "sigma must not be NULL")]
    else:
        cases += [(dict(which=2), "which"), (dict(which=-1), "which")]
    for kw, text in cases:
        rc, msg = _call(L, entry, **kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    # nothing wrong but the context: the last check that needs no device (2^28 points exactly is within the limit; negative steps are allowed)
    for kw in (dict(), dict(step=(-0.5, 0.1, 1e-3)), dict(iso=-3.0), dict(dims=(1024, 1024, 256)), dict(dims=(2, 2, 2))):
        rc, msg = _call(L, entry, **kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)


def test_python_layer_checks_shapes_without_a_device(native):
    net = native.Network(renderer=None, which=1)                  # never reaches the library
    with pytest.raises(native.NerfError):
        net.extract_mesh((0, 0), (1, 1, 1), (2, 2, 2), 1.0)
    with pytest.raises(native.NerfError):
        net.extract_mesh((0, 0, 0), (1, 1, 1), (2, 2.5, 2), 1.0)
    with pytest.raises(native.NerfError):
        native.isosurface(None, np.zeros((4, 4), F), (0, 0, 0), (1, 1, 1), 0.0)
    with pytest.raises(native.NerfError):
        native.save_ply("unused.ply", np.zeros((3, 3), F), np.zeros((1, 3), np.uint32), normals=np.zeros((2, 3), F))


# ---- PLY round trip ---------------------------------------------------------------------------------------------------------------------------
def parse_ply(raw):
    """A reader for what nerf_save_ply documents -> (vertices, normals or None, colours (uint8) or None, triangles)."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements, props = [], {}
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2]))); props[w[1]] = []
        elif w[0] == "property":
            props[elements[-1][0]].append(tuple(w[1:]))
        else:
            assert w[0] == "comment", ln
    assert [e[0] for e in elements] == ["vertex", "face"]
    assert props["face"] == [("list", "uchar", "uint", "vertex_indices")]
    names = [p[1] for p in props["vertex"]]
    assert all(p[0] == ("uchar" if p[1] in ("red", "green", "blue") else "float") for p in props["vertex"])
    assert names[:3] == ["x", "y", "z"] and names[3:] in ([], ["nx", "ny", "nz"], ["red", "green", "blue"], ["nx", "ny", "nz", "red", "green", "blue"])
    dt = np.dtype([(n, "u1" if n in ("red", "green", "blue") else "<f4") for n in names])
    nv, nt = elements[0][1], elements[1][1]
    body = raw[end:]
    assert len(body) == nv * dt.itemsize + nt * 13, (len(body), nv, dt.itemsize, nt)
    vert = np.frombuffer(body[:nv * dt.itemsize], dt)
    face = np.frombuffer(body[nv * dt.itemsize:], np.dtype([("n", "u1"), ("i", "<u4", 3)]))
    assert (face["n"] == 3).all()
    col = lambda ns: np.stack([vert[n] for n in ns], axis=1) if nv else np.zeros((0, 3), vert[ns[0]].dtype)
    return (col(["x", "y", "z"]), col(["nx", "ny", "nz"]) if "nx" in names else None, col(["red", "green", "blue"]) if "red" in names else None,
            face["i"].astype(np.uint32).reshape(-1, 3))


@pytest.mark.parametrize("with_colours", [False, True], ids=["plain", "colours"])
@pytest.mark.parametrize("with_normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("n_vertices,n_triangles", [(9, 8), (5000, 9001), (4, 0), (0, 0)])
def test_ply_round_trip(native, tmp_path, n_vertices, n_triangles, with_normals, with_colours):
    rng = np.random.default_rng(7 * n_vertices + n_triangles)
    v = rng.standard_normal((n_vertices, 3)).astype(F)
    n = rng.standard_normal((n_vertices, 3)).astype(F) if with_normals else None
    c = rng.uniform(-0.2, 1.2, (n_vertices, 3)).astype(F) if with_colours else None
    if with_colours and n_vertices:
        c[0] = [np.nan, 0.0, 1.0]
    t = rng.integers(0, max(n_vertices, 1), (n_triangles, 3)).astype(np.uint32)
    path = tmp_path / "m.ply"
    native.save_ply(path, v, t, normals=n, colours=c)
    gv, gn, gc, gt = parse_ply(path.read_bytes())
    assert np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gt, t)
    assert (gn is None) == (n is None) and (gn is None or np.array_equal(gn.view(np.uint32), n.view(np.uint32)))
    assert (gc is None) == (c is None) and (gc is None or np.array_equal(gc, native.quantize_rgb8(c)))


def test_ply_refusals(native, tmp_path):
    L = native.load_library()
    from nerf_rs_amd import _lib
    v = np.zeros((3, 3), F); t = np.array([[0, 1, 3]], np.uint32)
    pv, pt = v.ctypes.data_as(_lib.f32p), t.ctypes.data_as(_lib.u32p)
    path = str(tmp_path / "x.ply").encode()
    assert L.nerf_save_ply(path, 3, pv, None, None, 1, pt) == INVALID and b"beyond n_vertices" in L.nerf_last_error(None)
    assert L.nerf_save_ply(path, 3, None, None, None, 0, None) == INVALID
    assert L.nerf_save_ply(path, 3, pv, None, None, 1, None) == INVALID
    assert L.nerf_save_ply(None, 0, None, None, None, 0, None) == INVALID
    assert not (tmp_path / "x.ply").exists()                      # refused before the file is created
    assert L.nerf_save_ply(str(tmp_path / "no" / "dir" / "x.ply").encode(), 3, pv, None, None, 0, None) == -2


def test_ply_writer_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "nerf-rs_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "host-asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=87", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for nv, nt, with_n, with_c, want in ((9, 8, 1, 1, 0), (9, 8, 0, 0, 0), (1, 1, 0, 1, 0), (4097, 4095, 1, 0, 0), (4, 0, 1, 1, 0), (0, 0, 0, 0, 0), (0, 0, 1, 1, 0)):
        p = subprocess.run([os.path.join(csrc, "build", "host_asan_driver"), "ply", str(tmp_path / "a.ply"), str(nv), str(nt), str(with_n), str(with_c)],
                           capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, f"{(nv, nt, with_n, with_c)}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
        assert p.stdout.strip().splitlines()[-1].startswith(f"ply rc={want} "), p.stdout
    p = subprocess.run([os.path.join(csrc, "build", "host_asan_driver"), "ply", str(tmp_path / "no" / "dir" / "a.ply"), "3", "1", "0", "0"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert p.returncode == 0 and "ply rc=-2 " in p.stdout and "ERROR: AddressSanitizer" not in p.stderr
