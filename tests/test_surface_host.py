"""Host side of the quantile-depth and point-cloud entry points (nerf_render_rays_quantiles[_device], nerf_render_rays_points[_device],
nerf_stage_ray_quantiles, nerf_stage_gather_points): exported symbols and ctypes signatures, every argument refusal -- made with a NULL
context, so that no GPU is needed: "ctx is NULL" is reported only when nothing else is wrong --, the Python layer's shape checks, and a
point cloud through the PLY writer (zero faces).  The refusals of nerf_render_rays apply unchanged (the cases of
tests/test_ray_batch_host.py, run here through the new symbols).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_ray_batch_host import CASES as RAY_CASES, _args  # noqa: E402  (the argument table, not its tests)

INVALID = -1
NAMES = ("nerf_render_rays_quantiles", "nerf_render_rays_quantiles_device", "nerf_render_rays_points", "nerf_render_rays_points_device",
         "nerf_stage_ray_quantiles", "nerf_stage_gather_points")
BACKGROUND_CASES = [c for c in RAY_CASES if "background" in c[0]]     # a points call has no background argument


def _ray_part(a, device, keep):
    from nerf_rs_amd import _lib

    def f(v):
        if v is None:
            return None
        v = np.ascontiguousarray(v, np.float32)
        keep.append(v)
        return v.ctypes.data if device else v.ctypes.data_as(_lib.f32p)

    idx = None if a["rng_index"] is None else np.ascontiguousarray(a["rng_index"], np.uint32)
    keep.append(idx)
    opts = None if a["opts"] is None else C.byref(a["opts"])
    return f, (None, f(a["origins"]), a["n_origins"], f(a["dirs"]), a["n_rays"], a["normalize"], a["near"], a["far"], f(a["bounds"]),
               None if idx is None else (idx.ctypes.data if device else idx.ctypes.data_as(_lib.u32p)), opts)


def _rows(a):
    return max(a["n_rays"], 1) if a["n_rays"] < 2 ** 20 else 1


def call_quantiles(L, a, device, quantiles=(0.5,), n_q=None, depth_q="given"):
    from nerf_rs_amd import _lib
    keep = []
    f, head = _ray_part(a, device, keep)
    bg = None if a["background"] is None else np.ascontiguousarray(a["background"], np.float32)
    qs = None if quantiles is None else np.ascontiguousarray(quantiles, np.float32)
    n_q = (0 if qs is None else qs.size) if n_q is None else n_q
    out = np.zeros((8, _rows(a)), np.float32) if depth_q == "given" else None
    args = head + (None if bg is None else bg.ctypes.data_as(_lib.f32p), f(a["rgb"]), f(a["depth"]), f(a["opacity"]),
                   None if qs is None else qs.ctypes.data_as(_lib.f32p), n_q, f(out))
    rc = L.nerf_render_rays_quantiles_device(*args, None, None) if device else L.nerf_render_rays_quantiles(*args, None)
    return rc, L.nerf_last_error(None).decode()


def call_points(L, a, device, quantile=0.5, min_opacity=0.5, h=0.0, capacity=None, xyz="given", normals=None):
    from nerf_rs_amd import _lib
    keep = []
    f, head = _ray_part(a, device, keep)
    cap = _rows(a) if capacity is None else capacity
    x = np.zeros((max(cap, 1), 3), np.float32) if xyz == "given" else None
    nrm = np.zeros((max(cap, 1), 3), np.float32) if normals == "given" else None
    cnt = C.c_size_t(77)
    args = head + (quantile, min_opacity, h, cap, f(x), f(a["rgb"]), f(nrm), None, None, None, C.byref(cnt))
    rc = L.nerf_render_rays_points_device(*args, None, None, None) if device else L.nerf_render_rays_points(*args, None)
    return rc, L.nerf_last_error(None).decode()


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    htext = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\s*\(", htext), name
        assert getattr(L, name) is not None and name in _lib.PROTOTYPES
        assert name in htext[htext.index("additive:"):]                              # listed in the ABI comment
    assert re.search(r"#define NERF_MAX_QUANTILES 8\b", htext)
    P = _lib.PROTOTYPES
    rays, rays_dev = P["nerf_render_rays"], P["nerf_render_rays_device"]
    # the arguments of nerf_render_rays / _device, then quantiles (host), n_q and the planes, before stats / stream, stats
    assert P["nerf_render_rays_quantiles"] == (C.c_int, rays[1][:-1] + [_lib.f32p, C.c_int, _lib.f32p] + rays[1][-1:])
    assert P["nerf_render_rays_quantiles_device"] == (C.c_int, rays_dev[1][:-2] + [_lib.f32p, C.c_int, C.c_void_p] + rays_dev[1][-2:])
    # the ray arguments and opts (11), then quantile, min_opacity, h, capacity, the six output arrays and the count
    pts, pts_dev = P["nerf_render_rays_points"], P["nerf_render_rays_points_device"]
    tail = [C.c_float, C.c_float, C.c_float, C.c_size_t]
    assert pts == (C.c_int, rays[1][:11] + tail + [_lib.f32p, _lib.f32p, _lib.f32p, _lib.u32p, _lib.f32p, _lib.f32p, C.POINTER(C.c_size_t)] + rays[1][-1:])
    assert pts_dev == (C.c_int, rays_dev[1][:11] + tail + [C.c_void_p] * 6 + [C.POINTER(C.c_size_t), C.c_void_p] + rays_dev[1][-2:])
    assert P["nerf_stage_ray_quantiles"] == (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, _lib.f32p, _lib.f32p, _lib.f32p, C.c_int, _lib.f32p])
    assert len(P["nerf_stage_gather_points"][1]) == 18
    assert L.nerf_abi_version() == 5                                                 # additive: the version stays
    for fn in ("point_cloud", "point_cloud_device", "render_image_points", "save_point_cloud_ply"):
        assert callable(getattr(native, fn)), fn
    assert callable(native.Renderer.stage_ray_quantiles) and callable(native.Renderer.stage_gather_points)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("over,message", RAY_CASES, ids=[f"{i}:{m[:24]}" for i, (_, m) in enumerate(RAY_CASES)])
def test_the_refusals_of_render_rays_apply_unchanged(native, over, message, device):
    L = native.load_library()
    rc, msg = call_quantiles(L, _args(**dict(over)), device, quantiles=(7.0,))       # ... and come before the new ones
    assert rc == INVALID and message in msg, (rc, msg)
    if (over, message) not in BACKGROUND_CASES:
        rc, msg = call_points(L, _args(**dict(over)), device, quantile=7.0)
        assert rc == INVALID and message in msg, (rc, msg)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_quantile_refusals_in_the_stated_order(native, device):
    L = native.load_library()
    for n_q in (0, -1, 9):
        rc, msg = call_quantiles(L, _args(), device, quantiles=(float("nan"),) * 9, n_q=n_q, depth_q=None)
        assert rc == INVALID and msg == "n_q must be between 1 and NERF_MAX_QUANTILES (8)", (n_q, msg)
    assert call_quantiles(L, _args(), device, quantiles=None, n_q=2)[1] == "quantiles must not be NULL"
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        rc, msg = call_quantiles(L, _args(), device, quantiles=(0.5, bad), depth_q=None)
        assert rc == INVALID and msg == "a quantile must be finite and lie in (0, 1]", (bad, msg)
    assert call_quantiles(L, _args(), device, depth_q=None) == (INVALID, "depth_q_out must not be NULL")
    for qs in ((0.5,), (1.0,), (1e-30, 0.25, 0.5, 0.5, 0.75, 0.9, 0.99, 1.0)):
        assert call_quantiles(L, _args(), device, quantiles=qs) == (INVALID, "ctx is NULL"), qs
    assert call_quantiles(L, _args(n=0, origins=None, dirs=None, rgb=None), device, depth_q=None) == (INVALID, "ctx is NULL")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_points_refusals_in_the_stated_order(native, device):
    L = native.load_library()
    for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        rc, msg = call_points(L, _args(), device, quantile=bad, min_opacity=-1.0)
        assert rc == INVALID and msg == "a quantile must be finite and lie in (0, 1]", (bad, msg)
    for bad in (-1e-6, 1.0000001, float("nan"), float("inf")):
        rc, msg = call_points(L, _args(), device, min_opacity=bad, h=-1.0)
        assert rc == INVALID and msg == "min_opacity must be finite and lie in [0, 1]", (bad, msg)
    for bad in (-1e-3, float("nan"), float("inf")):
        rc, msg = call_points(L, _args(), device, h=bad, xyz=None)
        assert rc == INVALID and "h (the central-difference step) must be finite and not negative" in msg, (bad, msg)
    assert call_points(L, _args(), device, xyz=None, normals="given") == (INVALID, "xyz_out must not be NULL")
    assert call_points(L, _args(), device, normals="given") == (INVALID, "normals_out needs h > 0")
    assert call_points(L, _args(), device, h=1e-3) == (INVALID, "h > 0 needs normals_out")
    assert call_points(L, _args(rgb=None), device)[1] == "origins, dirs and rgb_out must not be NULL"
    for kw in (dict(), dict(min_opacity=0.0), dict(min_opacity=1.0, quantile=1.0), dict(h=1e-3, normals="given"), dict(capacity=0, xyz=None)):
        assert call_points(L, _args(), device, **kw) == (INVALID, "ctx is NULL"), kw
    assert call_points(L, _args(n_origins=4), device) == (INVALID, "ctx is NULL")


def test_a_bad_ray_is_named_after_the_new_arguments_are_checked(native):
    L = native.load_library()
    a = _args(n=6); a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan
    assert call_quantiles(L, a, False)[1].startswith("ray 2: its direction is not finite")
    assert call_points(L, a, False)[1].startswith("ray 2: its direction is not finite")
    assert call_quantiles(L, a, False, quantiles=(2.0,))[1].startswith("a quantile must be")
    assert call_points(L, a, False, min_opacity=2.0)[1].startswith("min_opacity must be")
    assert call_quantiles(L, a, True)[1] == "ctx is NULL" and call_points(L, a, True)[1] == "ctx is NULL"    # the device forms cannot look at the rays


def test_stage_call_refusals(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    p = lambda v: None if v is None else v.ctypes.data_as(_lib.f32p)  # noqa: E731
    w, t, out = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32), np.zeros((8, 4), np.float32)

    def quant(n_rays=4, n=8, w=w, t=t, qs=np.float32([0.5]), n_q=1, out=out):
        return L.nerf_stage_ray_quantiles(None, n_rays, n, p(w), p(t), p(qs), n_q, p(out)), L.nerf_last_error(None).decode()

    assert quant(n_q=0)[1].startswith("n_q must be") and quant(n_q=9)[1].startswith("n_q must be")
    assert quant(qs=None)[1] == "quantiles must not be NULL"
    assert quant(qs=np.float32([0.0]))[1].startswith("a quantile must be") and quant(qs=np.float32([np.nan]))[1].startswith("a quantile must be")
    assert quant(n=0)[1] == "n must be positive" and quant(n_rays=2 ** 31, n=2)[1] == "too many samples"
    assert quant(w=None)[1] == "NULL buffer" and quant(t=None)[1] == "NULL buffer" and quant(out=None)[1] == "NULL buffer"
    assert quant() == (INVALID, "ctx is NULL") and quant(n_rays=0, w=None, t=None, out=None) == (INVALID, "ctx is NULL")

    o, d, dq, c, a = np.zeros(3, np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    xyz, rgb, nrm = (np.zeros(3 * 4 + 64, np.float32) for _ in range(3))
    cnt = C.c_size_t(0)

    def gather(n_rays=4, n_origins=1, o=o, dq=dq, normals=None, min_opacity=0.5, capacity=4, xyz=xyz, normals_out=None, count=cnt):
        rc = L.nerf_stage_gather_points(None, n_rays, p(o), n_origins, p(d), p(dq), p(c), p(a), p(normals), min_opacity, capacity, p(xyz), p(rgb),
                                        p(normals_out), None, None, None, None if count is None else C.byref(count))
        return rc, L.nerf_last_error(None).decode()

    assert gather(n_rays=2 ** 31)[1] == "n_rays must be at most INT32_MAX" and gather(n_origins=2)[1].startswith("n_origins must be 1")
    assert gather(min_opacity=1.5)[1].startswith("min_opacity must be") and gather(min_opacity=float("nan"))[1].startswith("min_opacity must be")
    assert gather(capacity=2 ** 31)[1] == "capacity must be at most INT32_MAX"
    assert gather(o=None)[1] == "NULL buffer" and gather(dq=None)[1] == "NULL buffer"
    assert gather(xyz=None)[1].startswith("xyz_out, rgb_out and n_points") and gather(count=None)[1].startswith("xyz_out, rgb_out and n_points")
    assert gather(normals=c)[1] == "normals and normals_out go together" and gather(normals_out=nrm)[1] == "normals and normals_out go together"
    assert gather() == (INVALID, "ctx is NULL") and gather(normals=c, normals_out=nrm) == (INVALID, "ctx is NULL")


def test_python_layer_checks_shapes_and_ranges_without_a_device(native):
    class FakeNet:
        renderer = None
        which = 0
    net = FakeNet()
    o, d = np.float32([0, 0, 4]), np.tile(np.float32([0, 0, -1]), (4, 1))
    for bad in ([], [0.5] * 9, [0.0], [1.5], [float("nan")], [[0.5]]):
        with pytest.raises(native.NerfError, match="quantile"):
            native.render_rays(net, net, o, d, 2.0, 6.0, 16, quantiles=bad)
    with pytest.raises(native.NerfError, match="plain batch only"):
        native.render_rays(net, net, o, d, 2.0, 6.0, 16, quantiles=[0.5], normals_h=1e-3)
    with pytest.raises(native.NerfError, match="plain batch only"):
        native.render_rays(net, net, o, d, 2.0, 6.0, 16, quantiles=[0.5], certify_zero=True)
    with pytest.raises(native.NerfError, match="go together"):
        native.render_rays_device(net, net, 0, 1, 0, 4, 2.0, 6.0, 16, 0, d_depth_q=1234)
    with pytest.raises(native.NerfError, match="go together"):
        native.render_rays_device(net, net, 0, 1, 0, 4, 2.0, 6.0, 16, 0, quantiles=[0.5])
    with pytest.raises(native.NerfError, match=r"dirs must be an \(n, 3\) array"):
        native.point_cloud(net, net, o, np.zeros((4, 2), np.float32), 2.0, 6.0, 16)
    with pytest.raises(native.NerfError, match="origins must have shape"):
        native.point_cloud(net, net, np.zeros((3, 3), np.float32), d, 2.0, 6.0, 16)
    with pytest.raises(native.NerfError, match="quantile must be finite"):
        native.point_cloud(net, net, o, d, 2.0, 6.0, 16, quantile=0.0)
    with pytest.raises(native.NerfError, match="min_opacity must be finite"):
        native.point_cloud(net, net, o, d, 2.0, 6.0, 16, min_opacity=1.5)
    for bad in (0.0, -1e-3, float("nan")):
        with pytest.raises(native.NerfError, match="normals_h must be finite and greater than 0"):
            native.point_cloud(net, net, o, d, 2.0, 6.0, 16, normals_h=bad)
    with pytest.raises(native.NerfError, match="capacity must not be negative"):
        native.point_cloud(net, net, o, d, 2.0, 6.0, 16, capacity=-1)
    with pytest.raises(native.NerfError, match="go together"):
        native.point_cloud_device(net, net, 0, 1, 0, 4, 2.0, 6.0, 16, 4, 0, 0, normals_h=1e-3)
    with pytest.raises(native.NerfError, match="w and t must be"):
        native.Renderer.stage_ray_quantiles(None, np.zeros((4, 8)), np.zeros((4, 7)), [0.5])
    with pytest.raises(native.NerfError, match=r"depth_q and opacity must be \(n,\) arrays"):
        native.Renderer.stage_gather_points(None, o, d, np.zeros(3), np.zeros((4, 3)), np.zeros(4))


@pytest.mark.parametrize("with_normals", [False, True])
def test_point_cloud_ply_round_trip(native, tmp_path, with_normals):
    rng = np.random.default_rng(3)
    n = 37
    cloud = dict(xyz=rng.normal(size=(n, 3)).astype(np.float32), rgb=rng.uniform(0, 1, (n, 3)).astype(np.float32))
    if with_normals:
        cloud["normals"] = rng.normal(size=(n, 3)).astype(np.float32)
    path = tmp_path / "cloud.ply"
    native.save_point_cloud_ply(path, cloud)
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode().splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0"
    assert f"element vertex {n}" in header and "element face 0" in header
    props = [ln.split()[-1] for ln in header if ln.startswith("property") and "list" not in ln]
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
    stride = 12 + (12 if with_normals else 0) + 3
    body = np.frombuffer(raw[end:], np.uint8)
    assert body.size == n * stride                                                   # the vertex block and not one face
    rows = body.reshape(n, stride)
    assert np.array_equal(rows[:, :12].copy().view("<f4"), cloud["xyz"])
    if with_normals:
        assert np.array_equal(rows[:, 12:24].copy().view("<f4"), cloud["normals"])
    assert np.array_equal(rows[:, -3:], native.quantize_rgb8(cloud["rgb"]).reshape(n, 3))
    native.save_point_cloud_ply(path, dict(xyz=np.zeros((0, 3), np.float32), rgb=np.zeros((0, 3), np.float32)))    # an empty cloud is a file too
    assert b"element vertex 0" in path.read_bytes()
