"""Host side of the ray-clipping entry points (nerf_occupancy_dilate, nerf_clip_rays, nerf_render_rays_clipped, their _device forms and
nerf_debug_clip_rays): exported symbols, and every refusal the header lists -- made with a NULL context, so that no GPU is needed: the
checks that need no context come first, and "ctx is NULL" is reported only when nothing else is wrong.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

INVALID = -1
NAMES = ("nerf_occupancy_dilate", "nerf_occupancy_dilate_device", "nerf_clip_rays", "nerf_clip_rays_device", "nerf_debug_clip_rays",
         "nerf_render_rays_clipped", "nerf_render_rays_clipped_device")


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    htext = open(os.path.join(ROOT, "include", "nerf_mi355x.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\s*\(", htext), name
        assert getattr(L, name) is not None and name in _lib.PROTOTYPES
        assert name in htext[htext.index("additive:"):]                              # listed in the ABI comment
    P = _lib.PROTOTYPES
    assert len(P["nerf_clip_rays_device"][1]) == len(P["nerf_clip_rays"][1]) + 1     # + stream
    assert len(P["nerf_debug_clip_rays"][1]) == len(P["nerf_clip_rays"][1])          # - ctx + n_refused_reads
    assert len(P["nerf_render_rays_clipped"][1]) == len(P["nerf_render_rays"][1]) + 6   # + occ_bits, lo, step, dims, hit_out, n_hit
    assert len(P["nerf_render_rays_clipped_device"][1]) == len(P["nerf_render_rays_clipped"][1]) + 1
    assert L.nerf_abi_version() == 5


def _grid(**over):
    g = dict(bits=np.zeros(5, np.uint32), lo=np.float32([-1, -1, -1]), step=np.float32([0.5, 0.5, 0.5]), dims=np.int32([4, 5, 6]))
    g.update(over)
    return g


def _rays(n=4, n_origins=1, **over):
    from nerf_rs_amd import _lib
    a = dict(origins=np.tile(np.float32([0.0, 0.0, 4.0]), (max(n_origins, 1), 1)), dirs=np.tile(np.float32([0.0, 0.0, -1.0]), (max(n, 1), 1)),
             n_origins=n_origins, n_rays=n, normalize=1, near=2.0, far=6.0, bounds=None, rng_index=None, background=None,
             bounds_out=np.zeros((max(n, 1), 2), np.float32), hit=np.zeros(max(n, 1), np.uint8), rgb=np.zeros((max(n, 1), 3), np.float32))
    opts = _lib.COpts()
    opts.n_coarse, opts.n_fine = 8, 16
    for k in [k for k in over if k.startswith("opts_")]:
        setattr(opts, k[5:], over.pop(k))
    a["opts"] = opts
    a.update(over)
    return a


def _ptr(v, device, kind):
    if v is None:
        return None
    return v.ctypes.data if device else v.ctypes.data_as(kind)


def _clip(L, g, a, entry):
    """entry: 'host', 'device' or 'debug' -> (rc, message)"""
    from nerf_rs_amd import _lib
    dev = entry == "device"
    f = lambda v: _ptr(None if v is None else np.ascontiguousarray(v, np.float32), dev, _lib.f32p)
    keep = [np.ascontiguousarray(v, np.float32) if v is not None else None for v in (a["origins"], a["dirs"], a["bounds"])]
    grid = (_ptr(g["bits"], dev, _lib.u32p), _ptr(g["lo"], False, _lib.f32p), _ptr(g["step"], False, _lib.f32p), _ptr(g["dims"], False, _lib.i32p))
    tail = (f(keep[0]), a["n_origins"], f(keep[1]), a["n_rays"], a["normalize"], a["near"], a["far"], f(keep[2]), f(a["bounds_out"]),
            _ptr(a["hit"], dev, _lib.u8p), None)
    if entry == "host":
        rc = L.nerf_clip_rays(None, *grid, *tail)
    elif entry == "device":
        rc = L.nerf_clip_rays_device(None, *grid, *tail, None)
    else:
        rc = L.nerf_debug_clip_rays(*grid, *tail, None)
    return rc, L.nerf_last_error(None).decode()


def _clipped(L, g, a, device):
    from nerf_rs_amd import _lib
    f = lambda v: _ptr(None if v is None else np.ascontiguousarray(v, np.float32), device, _lib.f32p)
    keep = [np.ascontiguousarray(v, np.float32) if v is not None else None for v in (a["origins"], a["dirs"], a["bounds"])]
    idx = None if a["rng_index"] is None else np.ascontiguousarray(a["rng_index"], np.uint32)
    bg = None if a["background"] is None else np.ascontiguousarray(a["background"], np.float32)
    opts = None if a["opts"] is None else C.byref(a["opts"])
    head = (None, _ptr(g["bits"], device, _lib.u32p), _ptr(g["lo"], False, _lib.f32p), _ptr(g["step"], False, _lib.f32p), _ptr(g["dims"], False, _lib.i32p),
            f(keep[0]), a["n_origins"], f(keep[1]), a["n_rays"], a["normalize"], a["near"], a["far"], f(keep[2]), _ptr(idx, device, _lib.u32p), opts,
            _ptr(bg, False, _lib.f32p), f(a["rgb"]), None, None, _ptr(a["hit"], device, _lib.u8p), None)
    rc = L.nerf_render_rays_clipped_device(*head, None, None) if device else L.nerf_render_rays_clipped(*head, None)
    return rc, L.nerf_last_error(None).decode()


GRID_REFUSALS = [
    (dict(bits=None), "must not be NULL"), (dict(lo=None), "must not be NULL"), (dict(step=None), "must not be NULL"), (dict(dims=None), "must not be NULL"),
    (dict(dims=np.int32([4, 0, 6])), "dims must be positive"), (dict(dims=np.int32([4, 5, -1])), "dims must be positive"),
    (dict(lo=np.float32([0, np.nan, 0])), "lo must be finite"), (dict(lo=np.float32([np.inf, 0, 0])), "lo must be finite"),
    (dict(step=np.float32([0.5, 0.0, 0.5])), "step must be finite and greater than 0"), (dict(step=np.float32([0.5, 0.5, -0.5])), "step must be finite"),
    (dict(step=np.float32([np.nan, 0.5, 0.5])), "step must be finite"), (dict(step=np.float32([0.5, np.inf, 0.5])), "step must be finite"),
    (dict(dims=np.int32([2048, 2048, 512])), "grid too large"), (dict(dims=np.int32([65536, 65536, 1])), "grid too large"),
]


@pytest.mark.parametrize("entry", ["host", "device", "debug"])
def test_clip_rays_refusals_need_no_device(native, entry):
    L = native.load_library()
    rc, msg = _clip(L, _grid(), _rays(), entry)
    if entry == "debug":
        assert rc == 0                                                    # the host diagnostic needs no context at all
    else:
        assert rc == INVALID and msg == "ctx is NULL"                     # nothing else is wrong
    for over, text in GRID_REFUSALS:
        rc, msg = _clip(L, _grid(**over), _rays(), entry)
        assert rc == INVALID and text in msg, (over, msg)
    for over, text in ((dict(origins=None), "must not be NULL"), (dict(dirs=None), "must not be NULL"), (dict(bounds_out=None), "must not be NULL"),
                       (dict(hit=None), "must not be NULL"), (dict(n_origins=2), "n_origins must be 1"), (dict(n_origins=0), "n_origins must be 1"),
                       (dict(n_rays=2 ** 31), "at most INT32_MAX"), (dict(near=np.nan), "must be finite"), (dict(far=np.inf), "must be finite"),
                       (dict(near=6.0, far=6.0), "far_ must be greater than near_")):
        rc, msg = _clip(L, _grid(), _rays(**over), entry)
        assert rc == INVALID and text in msg, (over, msg)
    # with per-ray bounds near_ / far_ are not looked at; the grid is checked before the rays
    rc, msg = _clip(L, _grid(), _rays(near=np.nan, far=np.nan, bounds=np.tile(np.float32([2, 6]), (4, 1))), entry)
    assert (rc == 0) if entry == "debug" else (msg == "ctx is NULL")
    rc, msg = _clip(L, _grid(dims=np.int32([0, 1, 1])), _rays(dirs=None), entry)
    assert rc == INVALID and "dims must be positive" in msg
    # no rays: nothing to do, nothing to refuse about the buffers
    rc, msg = _clip(L, _grid(), _rays(n=0, origins=None, dirs=None, bounds_out=None, hit=None, n_origins=1), entry)
    assert (rc == 0) if entry == "debug" else (msg == "ctx is NULL")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_dilate_refusals_need_no_device(native, device):
    from nerf_rs_amd import _lib
    L = native.load_library()

    def call(bits, dims, radius, out):
        args = (None, _ptr(bits, device, _lib.u32p), _ptr(dims, False, _lib.i32p), radius, _ptr(out, device, _lib.u32p), None, None)
        rc = L.nerf_occupancy_dilate_device(*args, None) if device else L.nerf_occupancy_dilate(*args)
        return rc, L.nerf_last_error(None).decode()

    dims = np.int32([4, 5, 6])                                            # 120 cells: 4 words
    buf = np.zeros(16, np.uint32)
    src, dst = buf[:4], buf[8:12]
    assert call(src, dims, 1, dst) == (INVALID, "ctx is NULL")
    for radius in (0, -1, 5, 100):
        rc, msg = call(src, dims, radius, dst)
        assert rc == INVALID and "radius must be 1, 2, 3 or 4" in msg
    for radius in (1, 2, 3, 4):
        assert call(src, dims, radius, dst)[1] == "ctx is NULL"
    for a, b, c in ((None, dims, dst), (src, None, dst), (src, dims, None)):
        rc, msg = call(a, b, 1, c)
        assert rc == INVALID and "must not be NULL" in msg
    for bad in ([0, 5, 6], [4, -2, 6], [4, 5, 0]):
        rc, msg = call(src, np.int32(bad), 1, dst)
        assert rc == INVALID and "dims must be positive" in msg
    rc, msg = call(src, np.int32([2048, 2048, 512]), 1, dst)
    assert rc == INVALID and "grid too large" in msg
    # in and out must not alias: the same buffer, and ranges that share a word
    for out in (src, buf[3:7], buf[1:5]):
        rc, msg = call(src, dims, 1, out)
        assert rc == INVALID and "must not overlap" in msg, msg
    assert call(src, dims, 1, buf[4:8])[1] == "ctx is NULL"               # adjacent is fine


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_clipped_render_refusals_need_no_device(native, device):
    L = native.load_library()
    assert _clipped(L, _grid(), _rays(), device) == (INVALID, "ctx is NULL")
    for over, text in GRID_REFUSALS:
        rc, msg = _clipped(L, _grid(**over), _rays(), device)
        assert rc == INVALID and text in msg, (over, msg)
    # nerf_render_rays' own refusals, unchanged and in front of the grid's
    own = [(dict(opts=None), "opts is NULL"), (dict(n_rays=2 ** 31), "at most INT32_MAX"), (dict(origins=None), "must not be NULL"),
           (dict(dirs=None), "must not be NULL"), (dict(rgb=None), "must not be NULL"), (dict(n_origins=3), "n_origins must be 1"),
           (dict(opts_crop_w=4), "crop_* must be 0"), (dict(opts_ssaa=2), "ssaa must be 0 or 1"), (dict(opts_band_count=2), "band_count must be 0 or 1"),
           (dict(opts_skip_empty=1), "not available for ray batches"), (dict(opts_skip_dead=1), "not available for ray batches"),
           (dict(opts_hybrid_sampling=1), "not available for ray batches"), (dict(opts_certify_zero=1), "not available for ray batches"),
           (dict(opts_n_coarse=0), "coarse samples per ray must be greater than 0"), (dict(opts_n_fine=-1), "fine samples per ray must be >= 0"),
           (dict(opts_mlp_dtype=9), "mlp_dtype"), (dict(near=np.nan), "must be finite"), (dict(near=7.0), "far_ must be greater than near_"),
           (dict(background=np.float32([0, np.inf, 0])), "background components must be finite")]
    for over, text in own:
        a = _rays(**over)
        rc, msg = _clipped(L, _grid(), a, device)
        assert rc == INVALID and text in msg, (over, msg)
        # ... the very message nerf_render_rays gives
        from test_ray_batch_host import _args, _call
        ref = _call(L, _args(**over), device)
        assert ref == (rc, msg), (over, ref, msg)
        rc, msg = _clipped(L, _grid(dims=np.int32([0, 1, 1])), a, device)  # and they come first
        assert text in msg
    # the per-ray host checks, after the grid's
    bad = _rays(dirs=np.float32([[0, 0, -1], [0, np.nan, -1], [0, 0, -1], [0, 0, -1]]))
    rc, msg = _clipped(L, _grid(), bad, device)
    assert (msg == "ctx is NULL") if device else (rc == INVALID and msg.startswith("ray 1: its direction is not finite"))
    rc, msg = _clipped(L, _grid(step=np.float32([0, 1, 1])), bad, device)
    assert rc == INVALID and "step must be finite" in msg
    zero = _rays(dirs=np.float32([[0, 0, -1], [0, 0, -1], [0, 0, 0], [0, 0, -1]]))
    rc, msg = _clipped(L, _grid(), zero, device)
    assert (msg == "ctx is NULL") if device else msg.startswith("ray 2: its direction is zero")


def test_python_layer_checks_shapes_without_a_device(native):
    class FakeNet:
        renderer = None

    bits = np.zeros(4, np.uint32)
    with pytest.raises(native.NerfError, match="ceil"):
        native.clip_rays(None, bits[:3], (0, 0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((2, 3)), 0, 1, debug_cpu=True)
    with pytest.raises(native.NerfError, match="dims must be three integers"):
        native.clip_rays(None, bits, (0, 0, 0), (1, 1, 1), (4, 5), (0, 0, 0), np.zeros((2, 3)), 0, 1, debug_cpu=True)
    with pytest.raises(native.NerfError, match="dirs must be"):
        native.clip_rays(None, bits, (0, 0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((2, 4)), 0, 1, debug_cpu=True)
    with pytest.raises(native.NerfError, match="origins must have shape"):
        native.clip_rays(None, bits, (0, 0, 0), (1, 1, 1), (4, 5, 6), np.zeros((3, 3)), np.zeros((2, 3)), 0, 1, debug_cpu=True)
    with pytest.raises(native.NerfError, match="bounds must be"):
        native.clip_rays(None, bits, (0, 0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((2, 3)), 0, 1, bounds=np.zeros((3, 2)), debug_cpu=True)
    with pytest.raises(native.NerfError, match="lo and step"):
        native.clip_rays(None, bits, (0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((2, 3)), 0, 1, debug_cpu=True)
    with pytest.raises(native.NerfError, match="rng_index must have one entry per ray"):
        native.render_rays_clipped(FakeNet(), FakeNet(), bits, (0, 0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((2, 3)), 0, 1, rng_index=[1, 2, 3])
    out, hit = native.clip_rays(None, bits, (0, 0, 0), (1, 1, 1), (4, 5, 6), (0, 0, 0), np.zeros((0, 3)), 0, 1, debug_cpu=True)[:2]
    assert out.shape == (0, 2) and hit.shape == (0,)
