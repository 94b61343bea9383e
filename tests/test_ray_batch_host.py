"""Host side of the ray-batch entry points (nerf_render_rays, nerf_render_rays_device): exported symbols and ctypes signatures, and every
argument check the header lists -- made with a NULL context, so that no GPU is needed: the checks that need no context come first, and
"ctx is NULL" is reported only when nothing else is wrong.  The host entry point additionally looks at every ray and names the first one
it refuses.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID = -1


def _args(n=4, n_origins=1, device=False, **over):
    """A valid call's arguments (name -> value) for n rays; `over` replaces entries ('opts' entries by field name via opts_*)."""
    from nerf_rs_amd import _lib
    a = dict(origins=np.tile(np.array([0.0, 0.0, 4.0], np.float32), (max(n_origins, 1), 1)),
             dirs=np.tile(np.array([0.0, 0.0, -1.0], np.float32), (max(n, 1), 1)), n_origins=n_origins, n_rays=n, normalize=1, near=2.0, far=6.0,
             bounds=None, rng_index=None, background=None, rgb=np.zeros((max(n, 1), 3), np.float32), depth=None, opacity=None)
    opts = _lib.COpts()
    opts.n_coarse, opts.n_fine = 8, 16
    for k in [k for k in over if k.startswith("opts_")]:
        setattr(opts, k[5:], over.pop(k))
    a["opts"] = opts
    a.update(over)
    return a


def _call(L, a, device=False):
    from nerf_rs_amd import _lib

    def f(v):
        if v is None:
            return None
        v = np.ascontiguousarray(v, np.float32)
        return v.ctypes.data if device else v.ctypes.data_as(_lib.f32p)

    keep = [a["origins"], a["dirs"], a["bounds"], a["background"], a["rgb"]]
    idx = None if a["rng_index"] is None else np.ascontiguousarray(a["rng_index"], np.uint32)
    bg = None if a["background"] is None else np.ascontiguousarray(a["background"], np.float32).ctypes.data_as(_lib.f32p)
    opts = None if a["opts"] is None else C.byref(a["opts"])
    head = (None, f(a["origins"]), a["n_origins"], f(a["dirs"]), a["n_rays"], a["normalize"], a["near"], a["far"], f(a["bounds"]),
            None if idx is None else (idx.ctypes.data if device else idx.ctypes.data_as(_lib.u32p)), opts, bg, f(a["rgb"]), f(a["depth"]), f(a["opacity"]))
    rc = L.nerf_render_rays_device(*head, None, None) if device else L.nerf_render_rays(*head, None)
    del keep
    return rc, L.nerf_last_error(None).decode()


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    htext = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for name in ("nerf_render_rays", "nerf_render_rays_device"):
        assert re.search(r"\bint " + name + r"\s*\(", htext), name
        assert getattr(L, name) is not None and name in _lib.PROTOTYPES
        assert name in htext[htext.index("additive:"):]                              # listed in the ABI comment
    host, dev = _lib.PROTOTYPES["nerf_render_rays"], _lib.PROTOTYPES["nerf_render_rays_device"]
    assert host[0] is C.c_int and dev[0] is C.c_int
    assert len(host[1]) == 16 and len(dev[1]) == 17                                  # the device form adds the stream
    assert host[1][0] is C.c_void_p and host[1][2] is C.c_size_t and host[1][4] is C.c_size_t and host[1][5] is C.c_int
    assert host[1][6] is C.c_float and host[1][7] is C.c_float and host[1][9] is _lib.u32p and host[1][-1] == C.POINTER(_lib.CStats)
    assert dev[1][:8] == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float]
    assert dev[1][-2] is C.c_void_p and dev[1][-1] == C.POINTER(_lib.CStats)
    assert L.nerf_abi_version() == 5                                                 # additive: the version stays
    assert callable(native.render_rays) and callable(native.render_rays_device)


CASES = [
    (dict(opts=None), "opts is NULL"),
    (dict(n_rays=2 ** 31), "n_rays must be at most INT32_MAX"),
    (dict(origins=None), "origins, dirs and rgb_out must not be NULL"),
    (dict(dirs=None), "origins, dirs and rgb_out must not be NULL"),
    (dict(rgb=None), "origins, dirs and rgb_out must not be NULL"),
    (dict(n_origins=0), "n_origins must be 1"),
    (dict(n_origins=3), "n_origins must be 1"),
    (dict(opts_crop_w=2), "crop_* must be 0"),
    (dict(opts_crop_h=2), "crop_* must be 0"),
    (dict(opts_crop_x0=1), "crop_* must be 0"),
    (dict(opts_crop_y0=1), "crop_* must be 0"),
    (dict(opts_ssaa=2), "ssaa must be 0 or 1"),
    (dict(opts_band_count=2), "band_count must be 0 or 1"),
    (dict(opts_skip_empty=1), "not available for ray batches"),
    (dict(opts_skip_dead=1), "not available for ray batches"),
    (dict(opts_hybrid_sampling=1), "not available for ray batches"),
    (dict(opts_certify_zero=1), "not available for ray batches"),
    (dict(opts_n_coarse=0), "coarse samples per ray must be greater than 0"),
    (dict(opts_n_coarse=-3), "coarse samples per ray must be greater than 0"),
    (dict(opts_n_fine=-1), "fine samples per ray must be >= 0"),
    (dict(opts_mlp_dtype=4), "mlp_dtype must be"),
    (dict(opts_mlp_dtype=-1), "mlp_dtype must be"),
    (dict(near=float("nan")), "near_ and far_ must be finite"),
    (dict(far=float("inf")), "near_ and far_ must be finite"),
    (dict(near=6.0, far=6.0), "far_ must be greater than near_"),
    (dict(near=6.0, far=2.0), "far_ must be greater than near_"),
    (dict(background=(0.0, float("nan"), 0.0)), "background components must be finite"),
    (dict(background=(float("inf"), 0.0, 0.0)), "background components must be finite"),
    (dict(opts_n_coarse=30000, opts_n_fine=30000), "too many samples per ray"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("over,message", CASES, ids=[f"{i}:{m[:24]}" for i, (_, m) in enumerate(CASES)])
def test_argument_errors_need_no_context(native, over, message, device):
    L = native.load_library()
    rc, msg = _call(L, _args(**dict(over)), device)
    assert rc == INVALID and message in msg, (rc, msg)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_valid_call_reports_the_missing_context_last(native, device):
    L = native.load_library()
    valid = [_args(), _args(n_origins=4), _args(bounds=np.tile(np.array([2.0, 6.0], np.float32), (4, 1)), near=float("nan"), far=0.0),
             _args(rng_index=np.arange(4)), _args(background=(0.0, 2.0, -1.0)), _args(opts_coarse_only=1, opts_n_fine=0),
             _args(n=0, origins=None, dirs=None, rgb=None), _args(n=0, n_origins=0)]       # an empty batch needs no arrays -- but still a context
    for a in valid:
        rc, msg = _call(L, a, device)
        assert rc == INVALID and msg == "ctx is NULL", (rc, msg)


def test_the_host_form_names_the_first_offending_ray(native):
    L = native.load_library()
    n = 6

    def bad(field, ray, value, **kw):
        a = _args(n=n, **kw)
        arr = np.array(a[field], np.float32, copy=True)
        arr[ray] = value
        a[field] = arr
        return _call(L, a, False)

    per_ray_bounds = dict(bounds=np.tile(np.array([2.0, 6.0], np.float32), (n, 1)))
    for (rc, msg), want in [
        (bad("origins", 0, (0.0, float("nan"), 4.0)), "ray 0: its origin is not finite"),
        (bad("origins", 3, (float("inf"), 0.0, 4.0), n_origins=n), "ray 3: its origin is not finite"),
        (bad("dirs", 2, (0.0, float("nan"), -1.0)), "ray 2: its direction is not finite"),
        (bad("dirs", 5, (0.0, 0.0, 0.0)), "ray 5: its direction is zero"),
        (bad("bounds", 1, (float("nan"), 6.0), **per_ray_bounds), "ray 1: its bounds are not finite"),
        (bad("bounds", 4, (3.0, 3.0), **per_ray_bounds), "ray 4: its far is not greater than its near"),
        (bad("bounds", 4, (5.0, 2.0), **per_ray_bounds), "ray 4: its far is not greater than its near"),
    ]:
        assert rc == INVALID and msg.startswith(want), (rc, msg, want)
    a = _args(n=n)                                                                     # two bad rays: the first is named
    a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][1] = np.nan; a["dirs"][4] = 0.0
    assert _call(L, a, False)[1].startswith("ray 1: ")
    rc, msg = bad("dirs", 5, (0.0, 0.0, 0.0), normalize=0)                             # a zero direction is the caller's promise without normalize
    assert rc == INVALID and msg == "ctx is NULL"
    # the device form cannot look at the rays (it is given device pointers): the same arguments pass its checks
    a = _args(n=n); a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan
    assert _call(L, a, True)[1] == "ctx is NULL"
    # an argument error of the call outranks a bad ray
    a = _args(n=n, opts_ssaa=3); a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan
    assert "ssaa must be 0 or 1" in _call(L, a, False)[1]


def test_python_layer_checks_shapes_without_a_device(native):
    class FakeNet:
        renderer = None
    net = FakeNet()
    d = np.zeros((5, 3), np.float32)
    for kw, what in [(dict(origins=np.zeros(2), dirs=d), "origins must have shape"), (dict(origins=np.zeros((4, 3)), dirs=d), "origins must have shape"),
                     (dict(origins=np.zeros(3), dirs=np.zeros((5, 2))), "dirs must be"), (dict(origins=np.zeros(3), dirs=d, bounds=np.zeros((5, 3))), "bounds must be"),
                     (dict(origins=np.zeros(3), dirs=d, rng_index=np.arange(4)), "rng_index must have")]:
        with pytest.raises(native.NerfError, match=what):
            native.render_rays(net, net, kw.pop("origins"), kw.pop("dirs"), 2.0, 6.0, 16, **kw)
