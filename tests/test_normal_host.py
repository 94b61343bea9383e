"""Host side of the four surface-normal entry points (nerf_density_gradient_batch[_device], nerf_render_rays_normals[_device]): exported
symbols and ctypes signatures, and every argument refusal -- made with a NULL context, so that no GPU is needed: the checks that need no
context come first and "ctx is NULL" is reported only when nothing else is wrong.  The refusals of nerf_render_rays apply to the normals
entry points unchanged (the cases of tests/test_ray_batch_host.py, run here through the new symbols).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_ray_batch_host import CASES as RAY_CASES, _args  # noqa: E402  (the argument table, not its tests)

INVALID = -1
NAMES = ("nerf_density_gradient_batch", "nerf_density_gradient_batch_device", "nerf_render_rays_normals", "nerf_render_rays_normals_device")


def _call(L, a, device, h=1e-3, normals="given"):
    from nerf_rs_amd import _lib

    def f(v):
        if v is None:
            return None
        v = np.ascontiguousarray(v, np.float32)
        keep.append(v)
        return v.ctypes.data if device else v.ctypes.data_as(_lib.f32p)

    keep = []
    idx = None if a["rng_index"] is None else np.ascontiguousarray(a["rng_index"], np.uint32)
    bg = None if a["background"] is None else np.ascontiguousarray(a["background"], np.float32)
    out = np.zeros((max(a["n_rays"], 1) if a["n_rays"] < 2 ** 20 else 1, 3), np.float32) if normals == "given" else None
    opts = None if a["opts"] is None else C.byref(a["opts"])
    head = (None, f(a["origins"]), a["n_origins"], f(a["dirs"]), a["n_rays"], a["normalize"], a["near"], a["far"], f(a["bounds"]),
            None if idx is None else (idx.ctypes.data if device else idx.ctypes.data_as(_lib.u32p)), opts,
            None if bg is None else bg.ctypes.data_as(_lib.f32p), f(a["rgb"]), f(a["depth"]), f(a["opacity"]), h, f(out))
    rc = L.nerf_render_rays_normals_device(*head, None, None) if device else L.nerf_render_rays_normals(*head, None)
    return rc, L.nerf_last_error(None).decode()


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    htext = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\s*\(", htext), name
        assert getattr(L, name) is not None and name in _lib.PROTOTYPES
        assert name in htext[htext.index("additive:"):]                              # listed in the ABI comment
    P = _lib.PROTOTYPES
    rays, rays_dev = P["nerf_render_rays"], P["nerf_render_rays_device"]
    host, dev = P["nerf_render_rays_normals"], P["nerf_render_rays_normals_device"]
    # the arguments of nerf_render_rays / _device, then h and the normals, before stats / stream, stats
    assert host[0] is C.c_int and host[1] == rays[1][:-1] + [C.c_float, _lib.f32p] + rays[1][-1:]
    assert dev[0] is C.c_int and dev[1] == rays_dev[1][:-2] + [C.c_float, C.c_void_p] + rays_dev[1][-2:]
    assert P["nerf_density_gradient_batch"] == (C.c_int, [C.c_void_p, C.c_int, _lib.f32p, C.c_size_t, C.c_float, _lib.f32p])
    assert P["nerf_density_gradient_batch_device"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p])
    assert L.nerf_abi_version() == 5                                                 # additive: the version stays
    assert callable(native.render_image_normals) and callable(native.Network.density_gradient)
    for env in ("NERF_GRADIENT_CHUNK", "NERF_DEBUG_NORMALS"):                        # the knobs nerf_create reads are documented
        assert env in htext


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("over,message", RAY_CASES, ids=[f"{i}:{m[:24]}" for i, (_, m) in enumerate(RAY_CASES)])
def test_the_refusals_of_render_rays_apply_unchanged(native, over, message, device):
    rc, msg = _call(native.load_library(), _args(**dict(over)), device)
    assert rc == INVALID and message in msg, (rc, msg)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_step_and_normals_refusals(native, device):
    L = native.load_library()
    for h in (0.0, -1e-3, float("nan"), float("inf"), float("-inf")):
        rc, msg = _call(L, _args(), device, h=h)
        assert rc == INVALID and "h (the central-difference step) must be finite and greater than 0" in msg, (h, rc, msg)
    rc, msg = _call(L, _args(), device, normals=None)
    assert rc == INVALID and msg == "normals_out must not be NULL", (rc, msg)
    rc, msg = _call(L, _args(opts_ssaa=2), device, h=0.0)                            # nerf_render_rays' own refusals come first
    assert "ssaa must be 0 or 1" in msg
    for a in (_args(), _args(n_origins=4), _args(opts_coarse_only=1, opts_n_fine=0), _args(n=0, origins=None, dirs=None, rgb=None)):
        rc, msg = _call(L, a, device, h=1e-30)                                       # any positive finite step, subnormal included
        assert rc == INVALID and msg == "ctx is NULL", (rc, msg)


def test_a_bad_ray_is_named_after_the_step_is_checked(native):
    L = native.load_library()
    a = _args(n=6); a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan
    assert _call(L, a, False)[1].startswith("ray 2: its direction is not finite")
    assert "h (the central-difference step)" in _call(L, a, False, h=-1.0)[1]
    assert _call(L, a, True)[1] == "ctx is NULL"                                     # the device form cannot look at the rays


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_gradient_batch_refusals(native, device):
    from nerf_rs_amd import _lib
    L = native.load_library()
    pts, grad = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32)

    def call(which=0, p=pts, n=4, h=1e-3, g=grad):
        f = (lambda v: None if v is None else v.ctypes.data) if device else (lambda v: None if v is None else v.ctypes.data_as(_lib.f32p))
        rc = (L.nerf_density_gradient_batch_device(None, which, f(p), n, h, f(g), None) if device
              else L.nerf_density_gradient_batch(None, which, f(p), n, h, f(g)))
        return rc, L.nerf_last_error(None).decode()

    for which in (-1, 2):
        assert call(which=which) == (INVALID, "which must be NERF_NET_COARSE or NERF_NET_FINE")
    for h in (0.0, -1.0, float("nan"), float("inf")):
        rc, msg = call(h=h)
        assert rc == INVALID and "must be finite and greater than 0" in msg, (h, msg)
    assert call(p=None) == (INVALID, "NULL buffer") and call(g=None) == (INVALID, "NULL buffer")
    assert call(which=3, h=0.0, p=None)[1].startswith("which must be")               # in the header's order
    assert call() == (INVALID, "ctx is NULL") and call(which=1) == (INVALID, "ctx is NULL")
    assert call(n=0, p=None, g=None) == (INVALID, "ctx is NULL")                     # an empty batch needs no arrays -- but still a context


def test_python_layer_checks_shapes_without_a_device(native):
    class FakeNet:
        renderer = None
        which = 0
    with pytest.raises(native.NerfError, match="points must be a 3 x B matrix"):
        native.Network.density_gradient(FakeNet(), np.zeros((4, 3), np.float32), 1e-3)
    with pytest.raises(native.NerfError, match="go together"):
        native.render_rays_device(FakeNet(), FakeNet(), 0, 1, 0, 4, 2.0, 6.0, 16, 0, d_normals=1234)
