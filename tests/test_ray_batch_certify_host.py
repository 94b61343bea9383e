"""Host side of the certified ray batches (nerf_render_rays_certified, nerf_render_rays_clipped_certified, their _device forms, and the
stage call nerf_stage_prefilter_rays): exported symbols and ctypes signatures, and every refusal of the four render calls, message by
message -- made with a NULL context, so that no GPU is needed: the checks that need no context come first, and "ctx is NULL" is reported
only when nothing else is wrong.  The table is the uncertified calls' (tests/test_ray_batch_host.py) with the certify_zero row replaced by
"accepted", plus the two refusals of the certified forms alone.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID = -1
CERTIFIED = ("nerf_render_rays_certified", "nerf_render_rays_certified_device", "nerf_render_rays_clipped_certified",
             "nerf_render_rays_clipped_certified_device")
PLAIN = ("nerf_render_rays", "nerf_render_rays_device", "nerf_render_rays_clipped", "nerf_render_rays_clipped_device")
FORMS = [("rays", False), ("rays", True), ("clipped", False), ("clipped", True)]
FORM_IDS = ["rays-host", "rays-device", "clipped-host", "clipped-device"]


def _args(n=4, n_origins=1, **over):
    """A valid call's arguments (name -> value) for n rays; `over` replaces entries ('opts' fields by name via opts_*)."""
    from nerf_rs_amd import _lib
    a = dict(origins=np.tile(np.float32([0.0, 0.0, 4.0]), (max(n_origins, 1), 1)), dirs=np.tile(np.float32([0.0, 0.0, -1.0]), (max(n, 1), 1)),
             n_origins=n_origins, n_rays=n, normalize=1, near=2.0, far=6.0, bounds=None, rng_index=None, background=None,
             rgb=np.zeros((max(n, 1), 3), np.float32), bits=np.zeros(5, np.uint32), lo=np.float32([-1, -1, -1]), step=np.float32([0.5, 0.5, 0.5]),
             dims=np.int32([4, 5, 6]))
    opts = _lib.COpts()
    opts.n_coarse, opts.n_fine = 8, 16
    for k in [k for k in over if k.startswith("opts_")]:
        setattr(opts, k[5:], over.pop(k))
    a["opts"] = opts
    a.update(over)
    return a


def _call(L, a, kind, device, certified=True):
    """One of the eight entry points with a NULL context -> (rc, message)."""
    from nerf_rs_amd import _lib

    def ptr(v, ctype, dev=device):
        if v is None:
            return None
        return v.ctypes.data if dev else v.ctypes.data_as(ctype)

    arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.float32) for k in ("origins", "dirs", "bounds", "background", "rgb")}
    idx = None if a["rng_index"] is None else np.ascontiguousarray(a["rng_index"], np.uint32)
    opts = None if a["opts"] is None else C.byref(a["opts"])
    rays = (ptr(arr["origins"], _lib.f32p), a["n_origins"], ptr(arr["dirs"], _lib.f32p), a["n_rays"], a["normalize"], a["near"], a["far"],
            ptr(arr["bounds"], _lib.f32p), ptr(idx, _lib.u32p), opts, ptr(arr["background"], _lib.f32p, False), ptr(arr["rgb"], _lib.f32p), None, None)
    if kind == "rays":
        name = "nerf_render_rays" + ("_certified" if certified else "") + ("_device" if device else "")
        head = (None,) + rays
    else:
        name = "nerf_render_rays_clipped" + ("_certified" if certified else "") + ("_device" if device else "")
        head = (None, ptr(a["bits"], _lib.u32p), ptr(a["lo"], _lib.f32p, False), ptr(a["step"], _lib.f32p, False), ptr(a["dims"], _lib.i32p, False)) + rays + (None, None)
    rc = getattr(L, name)(*head, None, None) if device else getattr(L, name)(*head, None)
    return rc, L.nerf_last_error(None).decode()


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    htext = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for name in CERTIFIED + ("nerf_stage_prefilter_rays",):
        assert re.search(r"\bint " + name + r"\s*\(", htext), name
        assert getattr(L, name) is not None and name in _lib.PROTOTYPES
        assert name in htext[htext.index("additive:"):]                              # listed in the ABI comment
    for cert, plain in zip(CERTIFIED, PLAIN):                                        # the argument list of the uncertified call
        assert _lib.PROTOTYPES[cert] == _lib.PROTOTYPES[plain] and _lib.PROTOTYPES[cert][1] is not _lib.PROTOTYPES[plain][1]
    assert _lib.PROTOTYPES["nerf_stage_prefilter_rays"] == _lib.PROTOTYPES["nerf_stage_prefilter"]
    assert L.nerf_abi_version() == 5                                                 # additive: the version stays
    assert "currently 5" in htext
    for fn in (native.render_rays, native.render_rays_device, native.render_rays_clipped, native.render_rays_clipped_device):
        assert fn.__kwdefaults__["certify_zero"] is False
    # the header says what the device forms do to the stream, and that nothing is expanded
    sec = htext[htext.index("int nerf_render_rays_device"):htext.index("int nerf_render_rays_certified_device")]
    assert "SYNCHRONISES `stream`" in sec and "no points are expanded" in sec


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
    (dict(opts_certify_zero=2), "certify_zero must be 0 or 1"),
    (dict(opts_certify_zero=-1), "certify_zero must be 0 or 1"),
    (dict(opts_n_coarse=0), "coarse samples per ray must be greater than 0"),
    (dict(opts_n_coarse=-3), "coarse samples per ray must be greater than 0"),
    (dict(opts_n_fine=-1), "fine samples per ray must be >= 0"),
    (dict(opts_mlp_dtype=4), "mlp_dtype must be"),
    (dict(opts_mlp_dtype=-1), "mlp_dtype must be"),
    (dict(opts_mlp_dtype=1), "certify_zero needs mlp_dtype F32, BF16X3 or F16X2"),      # NERF_MLP_BF16
    (dict(opts_mlp_dtype=1, opts_certify_zero=1), "certify_zero needs"),
    (dict(near=float("nan")), "near_ and far_ must be finite"),
    (dict(far=float("inf")), "near_ and far_ must be finite"),
    (dict(near=6.0, far=6.0), "far_ must be greater than near_"),
    (dict(near=6.0, far=2.0), "far_ must be greater than near_"),
    (dict(background=(0.0, float("nan"), 0.0)), "background components must be finite"),
    (dict(background=(float("inf"), 0.0, 0.0)), "background components must be finite"),
    (dict(opts_n_coarse=30000, opts_n_fine=30000), "too many samples per ray"),
]


@pytest.mark.parametrize("kind,device", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("over,message", CASES, ids=[f"{i}:{m[:24]}" for i, (_, m) in enumerate(CASES)])
def test_argument_errors_need_no_context(native, over, message, kind, device):
    L = native.load_library()
    rc, msg = _call(L, _args(**dict(over)), kind, device)
    assert rc == INVALID and message in msg, (rc, msg)


@pytest.mark.parametrize("kind,device", FORMS, ids=FORM_IDS)
def test_a_valid_call_reports_the_missing_context_last(native, kind, device):
    L = native.load_library()
    valid = [_args(), _args(opts_certify_zero=1),                                      # the entry point is the switch: 0 and 1 are both accepted
             _args(n_origins=4), _args(bounds=np.tile(np.float32([2.0, 6.0]), (4, 1)), near=float("nan"), far=0.0),
             _args(rng_index=np.arange(4)), _args(background=(0.0, 2.0, -1.0)), _args(opts_coarse_only=1, opts_n_fine=0),
             _args(opts_mlp_dtype=2), _args(opts_mlp_dtype=3),                         # BF16X3, F16X2
             _args(n=0, origins=None, dirs=None, rgb=None), _args(n=0, n_origins=0)]   # an empty batch needs no arrays -- but still a context
    for a in valid:
        rc, msg = _call(L, a, kind, device)
        assert rc == INVALID and msg == "ctx is NULL", (rc, msg)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_clipped_form_checks_the_grid_after_the_batch(native, device):
    L = native.load_library()
    for over, text in ((dict(bits=None), "must not be NULL"), (dict(dims=np.int32([4, 0, 6])), "dims must be positive"),
                       (dict(step=np.float32([0.5, 0.0, 0.5])), "step must be finite and greater than 0")):
        rc, msg = _call(L, _args(**over), "clipped", device)
        assert rc == INVALID and text in msg, (over, msg)
    rc, msg = _call(L, _args(dims=np.int32([4, 0, 6]), opts_mlp_dtype=1), "clipped", device)   # the batch's refusals come first
    assert rc == INVALID and "certify_zero needs" in msg


def test_the_host_forms_name_the_first_offending_ray(native):
    L = native.load_library()
    for kind in ("rays", "clipped"):
        a = _args(n=6)
        a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan; a["dirs"][4] = 0.0
        assert _call(L, a, kind, False)[1].startswith("ray 2: its direction is not finite")
        assert _call(L, a, kind, True)[1] == "ctx is NULL"                             # the device form cannot look at the rays
        a = _args(n=6, opts_ssaa=3); a["dirs"] = np.array(a["dirs"], copy=True); a["dirs"][2] = np.nan
        assert "ssaa must be 0 or 1" in _call(L, a, kind, False)[1]                    # an argument error outranks a bad ray


@pytest.mark.parametrize("kind,device", FORMS, ids=FORM_IDS)
def test_the_existing_entry_points_still_refuse_certify_zero(native, kind, device):
    L = native.load_library()
    rc, msg = _call(L, _args(opts_certify_zero=1), kind, device, certified=False)
    assert rc == INVALID and "skip_empty, skip_dead, hybrid_sampling and certify_zero are not available for ray batches (first version)" in msg
    rc, msg = _call(L, _args(), kind, device, certified=False)
    assert rc == INVALID and msg == "ctx is NULL"


def test_python_layer_refuses_normals_on_a_certified_batch(native):
    class FakeNet:
        renderer = None
    net = FakeNet()
    with pytest.raises(native.NerfError, match="normals are not offered"):
        native.render_rays(net, net, np.zeros(3), np.zeros((5, 3)), 2.0, 6.0, 16, normals_h=1e-3, certify_zero=True)
    with pytest.raises(native.NerfError, match="give either origin or origins"):
        native.Renderer.stage_prefilter(None, 0, None, np.zeros((2, 3)), np.zeros((2, 8)), 6.0)


def test_stage_prefilter_rays_refusals_need_no_context(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    n, spr = 3, 8
    o, d, t = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, spr), np.float32)
    out, bad = np.zeros((n, spr), np.float32), np.zeros(1, np.uint32)
    p = lambda v: None if v is None else v.ctypes.data_as(_lib.f32p)

    def call(which=0, origins=o, spr_=spr, cut=0.0):
        rc = L.nerf_stage_prefilter_rays(None, which, 1, p(origins), p(d), p(t), n, spr_, 6.0, cut, p(out), bad.ctypes.data_as(_lib.u32p))
        return rc, L.nerf_last_error(None).decode()

    assert call() == (INVALID, "ctx is NULL")
    assert "which must be" in call(which=2)[1] and "spr must be positive" in call(spr_=0)[1]
    assert "cut_T must lie in [0, 1)" in call(cut=1.0)[1] and "NULL buffer" in call(origins=None)[1]
