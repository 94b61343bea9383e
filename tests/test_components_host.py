"""Lattice components, host side (no device): the five entry points exist with their ctypes signatures; the two structs have the sizes the
header states; every argument error is refused before anything touches a context or a device (a NULL context reaches them, and "ctx is NULL"
is the last refusal); and the header, the Python loader, the Rust crates, the CLI and the documents all name the same things."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FUNCTIONS = ("nerf_lattice_components", "nerf_lattice_components_device", "nerf_isosurface_grid_filtered", "nerf_extract_mesh_filtered",
             "nerf_extract_mesh_filtered_device")
INVALID = -1
F = np.float32


def test_symbols_signatures_and_struct_sizes(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    f32p, u32p, i32p, u64p, vp, sz = _lib.f32p, _lib.u32p, _lib.i32p, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t
    want = {
        "nerf_lattice_components": [vp, f32p, i32p, C.c_float, u32p, vp, sz, u64p],
        "nerf_lattice_components_device": [vp, vp, i32p, C.c_float, vp, vp, sz, u64p, vp],
        "nerf_isosurface_grid_filtered": [vp, f32p, f32p, f32p, i32p, C.c_float, vp, f32p, f32p, sz, u32p, sz, u64p, u64p, u64p, u64p],
        "nerf_extract_mesh_filtered": [vp, C.c_int, f32p, f32p, i32p, C.c_float, vp, f32p, f32p, f32p, sz, u32p, sz, u64p, u64p, u64p, u64p],
        "nerf_extract_mesh_filtered_device": [vp, C.c_int, f32p, f32p, i32p, C.c_float, vp, vp, vp, vp, sz, vp, sz, u64p, u64p, u64p, u64p, vp],
    }
    for name in FUNCTIONS:
        fn = getattr(L, name)                                    # AttributeError without the feature
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args == want[name], name
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    assert L.nerf_abi_version() == 5                              # additive
    assert C.sizeof(_lib.CComponentFilter) == 8 and C.sizeof(_lib.CComponent) == 32
    assert [f[0] for f in _lib.CComponentFilter._fields_] == ["keep_largest", "min_points"]
    assert [f[0] for f in _lib.CComponent._fields_] == ["label", "n_points", "bounds"] and _lib.CComponent.bounds.offset == 8
    assert callable(native.lattice_components) and callable(native.lattice_components_device) and native.Component._fields == ("label", "n_points", "bounds")
    import inspect
    for fn in (native.isosurface, native.Network.extract_mesh, native.Network.extract_mesh_device):
        p = inspect.signature(fn).parameters
        assert p["keep_largest"].default == 0 and p["min_points"].default == 0, fn


def test_header_states_the_struct_layouts():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read(), flags=re.S)
    assert re.search(r"typedef struct \{\s*uint32_t keep_largest, min_points;\s*\}\s*nerf_component_filter;", text)
    assert re.search(r"typedef struct \{\s*uint32_t label, n_points;\s*int32_t bounds\[6\];\s*\}\s*nerf_component;", text)


def _components(L, ctx=None, sigma=True, dims=(3, 3, 3), iso=1.0, table=True, cap=4, count=True, device=False):
    from nerf_rs_amd import _lib
    sig = np.zeros(64, F); labels = np.zeros(64, np.uint32); tab = (_lib.CComponent * 64)()
    n = C.c_uint64()
    i3 = None if dims is None else C.cast((C.c_int32 * 3)(*dims), _lib.i32p)
    if device:
        rc = L.nerf_lattice_components_device(ctx, sig.ctypes.data if sigma else None, i3, iso, labels.ctypes.data, C.addressof(tab) if table else None, cap,
                                              C.byref(n) if count else None, None)
    else:
        rc = L.nerf_lattice_components(ctx, sig.ctypes.data_as(_lib.f32p) if sigma else None, i3, iso, labels.ctypes.data_as(_lib.u32p),
                                       C.addressof(tab) if table else None, cap, C.byref(n) if count else None)
    return rc, L.nerf_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_component_argument_errors_need_no_device(native, device):
    L = native.load_library()
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(sigma=False), "sigma must not be NULL"), (dict(dims=None), "dims must not be NULL"), (dict(count=False), "required"),
        (dict(dims=(0, 3, 3)), "positive"), (dict(dims=(3, -1, 3)), "positive"), (dict(dims=(3, 3, 0)), "positive"),
        (dict(iso=nan), "finite"), (dict(iso=inf), "finite"), (dict(iso=-inf), "finite"),
        (dict(cap=65), "at most 64"), (dict(cap=2 ** 40), "at most 64"), (dict(cap=0), "cap_table > 0"),
        (dict(dims=(1024, 1024, 257)), "too large"), (dict(dims=(65536, 65536, 2)), "too large"), (dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "too large"),
    ]
    for kw, text in cases:
        rc, msg = _components(L, device=device, **kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    # nothing wrong but the context: dims of 1 are allowed here, 2^28 points exactly are within the limit, a table is optional
    for kw in (dict(), dict(dims=(1, 1, 1)), dict(dims=(1024, 1024, 256)), dict(table=False, cap=0), dict(table=False, cap=7), dict(cap=64), dict(iso=-2.5)):
        rc, msg = _components(L, device=device, **kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)


def _filtered(L, entry, filt, ctx=None, dims=(3, 3, 3), iso=1.0, step=(0.1, 0.1, 0.1)):
    from nerf_rs_amd import _lib
    sig = np.zeros(64, F); v = np.zeros((8, 3), F); n = np.zeros((8, 3), F); c = np.zeros((8, 3), F); t = np.zeros((8, 3), np.uint32)
    nv, nt, nc, nk = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    f3 = lambda a: C.cast((C.c_float * 3)(*a), _lib.f32p)
    i3 = C.cast((C.c_int32 * 3)(*dims), _lib.i32p)
    f = None if filt is None else _lib.CComponentFilter(*filt)
    pf = None if f is None else C.addressof(f)
    if entry == "grid":
        rc = L.nerf_isosurface_grid_filtered(ctx, sig.ctypes.data_as(_lib.f32p), f3((0, 0, 0)), f3(step), i3, iso, pf, v.ctypes.data_as(_lib.f32p),
                                             n.ctypes.data_as(_lib.f32p), 8, t.ctypes.data_as(_lib.u32p), 8, C.byref(nv), C.byref(nt), C.byref(nc), C.byref(nk))
    elif entry == "net":
        rc = L.nerf_extract_mesh_filtered(ctx, 1, f3((0, 0, 0)), f3(step), i3, iso, pf, v.ctypes.data_as(_lib.f32p), n.ctypes.data_as(_lib.f32p),
                                          c.ctypes.data_as(_lib.f32p), 8, t.ctypes.data_as(_lib.u32p), 8, C.byref(nv), C.byref(nt), None, None)
    else:
        rc = L.nerf_extract_mesh_filtered_device(ctx, 1, f3((0, 0, 0)), f3(step), i3, iso, pf, v.ctypes.data, n.ctypes.data, c.ctypes.data, 8, t.ctypes.data, 8,
                                                 C.byref(nv), C.byref(nt), C.byref(nc), None, None)
    return rc, L.nerf_last_error(None).decode()


@pytest.mark.parametrize("entry", ["grid", "net", "device"])
def test_filter_argument_errors_need_no_device(native, entry):
    L = native.load_library()
    for filt in ((65, 0), (2 ** 32 - 1, 0), (1000, 5)):
        rc, msg = _filtered(L, entry, filt)
        assert rc == INVALID and "keep_largest" in msg, (filt, rc, msg)
    # the mesh entry points' own refusals still come before the context is needed
    for kw, text in ((dict(dims=(1, 3, 3)), "at least 2"), (dict(iso=float("nan")), "finite"), (dict(step=(0.1, 0.0, 0.1)), "step must not be 0"),
                     (dict(dims=(1024, 1024, 257)), "too large")):
        rc, msg = _filtered(L, entry, (1, 0), **kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    for filt in (None, (0, 0), (1, 0), (64, 0), (0, 2 ** 32 - 1), (64, 17)):
        rc, msg = _filtered(L, entry, filt)
        assert rc == INVALID and msg == "ctx is NULL", (filt, rc, msg)


def test_python_layer_checks_without_a_device(native):
    with pytest.raises(native.NerfError):
        native.lattice_components(None, np.zeros((4, 4), F), 0.0)
    with pytest.raises(native.NerfError):
        native.lattice_components(None, np.zeros((2, 2, 2), F), 0.0, table=-1)
    with pytest.raises(native.NerfError):
        native.isosurface(None, np.zeros((2, 2, 2), F), (0, 0, 0), (1, 1, 1), 0.0, keep_largest=-1)
    with pytest.raises(native.NerfError):
        native.lattice_components_device(None, 0, (2, 2), 0.0)


def test_every_layer_names_the_feature():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    header = read("include", "nerf_mi355x.h")
    sys_rs, safe_rs, cli_rs = (read("bindings", "rust", d, "src", f) for d, f in (("nerf-mi355x-sys", "lib.rs"), ("nerf-mi355x", "lib.rs"), ("nerf-mi355x-cli", "main.rs")))
    integration, readme, design, cli = read("INTEGRATION.md"), read("README.md"), read("DESIGN.md"), read("nerf-rs_amd", "csrc", "nerf_cli.cpp")
    for name in FUNCTIONS:
        assert name in header and f"pub fn {name}" in sys_rs, name
    for name in ("nerf_lattice_components", "nerf_extract_mesh_filtered"):
        assert f"pub fn {name}" in integration and name in safe_rs, name
    for struct in ("nerf_component_filter", "nerf_component"):
        assert f"pub struct {struct} " in sys_rs and struct in header, struct
    assert "size_of::<nerf_component_filter>() == 8" in sys_rs and "size_of::<nerf_component>() == 32" in sys_rs
    for flag in ("--mesh-keep-largest", "--mesh-min-points"):
        assert flag in cli and flag in cli_rs and flag in readme, flag
    assert "4.12" in design and "nerf_lattice_components" in design and "lattice components" in header
    for text in (header, design):
        assert "0xFFFFFFFF" in text and "14" in text                 # the label of an outside point, the 14 neighbours
