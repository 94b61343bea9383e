"""Density queries, host side (no device): the four entry points exist with the ctypes signatures, every argument error the header lists
is refused before anything touches a device -- the checks that need no context come first, so they can be told apart by their messages
even with a NULL context -- and unpack_occupancy decodes hand-written words."""
import ctypes as C

import numpy as np
import pytest

DENSITY_FUNCTIONS = ("nerf_density_batch", "nerf_density_batch_device", "nerf_density_grid", "nerf_density_grid_device")
INVALID = -1


def _f3(*v):
    return (C.c_float * 3)(*v)


def _i3(*v):
    return (C.c_int32 * 3)(*v)


def _cast(a, t):
    return C.cast(a, t)


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    f32p, u32p, i32p, u64p, vp = _lib.f32p, _lib.u32p, _lib.i32p, C.POINTER(C.c_uint64), C.c_void_p
    want = {
        "nerf_density_batch": [vp, C.c_int, f32p, C.c_size_t, f32p],
        "nerf_density_batch_device": [vp, C.c_int, vp, C.c_size_t, vp, vp],
        "nerf_density_grid": [vp, C.c_int, f32p, f32p, i32p, f32p, C.c_float, u32p, u64p, i32p],
        "nerf_density_grid_device": [vp, C.c_int, f32p, f32p, i32p, vp, C.c_float, vp, u64p, i32p, vp],
    }
    for name in DENSITY_FUNCTIONS:
        fn = getattr(L, name)                                    # AttributeError without the feature
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args == want[name], name
        assert fn.restype is C.c_int and list(fn.argtypes) == want[name], name
    for name in ("density", "density_device", "density_grid", "density_grid_device"):
        assert callable(getattr(native.Network, name)), name
    assert callable(native.unpack_occupancy)


def _grid(L, device, ctx=None, which=1, lo=(0.0, 0.0, 0.0), step=(0.1, 0.1, 0.1), dims=(2, 2, 2), sigma=True, thr=0.0, bits=True, count=False,
          bounds=False):
    """One call with real (small) host buffers; returns (rc, message)."""
    from nerf_rs_amd import _lib
    sig = np.zeros(64, np.float32); words = np.zeros(8, np.uint32); cnt = C.c_uint64(); bnd = np.zeros(6, np.int32)
    args = [ctx, which, _cast(_f3(*lo), _lib.f32p) if lo is not None else None, _cast(_f3(*step), _lib.f32p) if step is not None else None,
            _cast(_i3(*dims), _lib.i32p) if dims is not None else None]
    if device:
        rc = L.nerf_density_grid_device(*args, sig.ctypes.data if sigma else None, thr, words.ctypes.data if bits else None,
                                        C.byref(cnt) if count else None, bnd.ctypes.data_as(_lib.i32p) if bounds else None, None)
    else:
        rc = L.nerf_density_grid(*args, sig.ctypes.data_as(_lib.f32p) if sigma else None, thr, words.ctypes.data_as(_lib.u32p) if bits else None,
                                 C.byref(cnt) if count else None, bnd.ctypes.data_as(_lib.i32p) if bounds else None)
    return rc, L.nerf_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_grid_argument_errors_need_no_device(native, device):
    L = native.load_library()
    inf, nan = float("inf"), float("nan")
    cases = [
        (dict(which=2), "which"), (dict(which=-1), "which"),
        (dict(dims=(0, 2, 2)), "dims must be positive"), (dict(dims=(2, -1, 2)), "dims must be positive"), (dict(dims=(2, 2, 0)), "dims must be positive"),
        (dict(dims=None), "must not be NULL"), (dict(lo=None), "must not be NULL"), (dict(step=None), "must not be NULL"),
        (dict(dims=(65536, 65536, 1)), "too large"), (dict(dims=(2048, 2048, 2048)), "too large"), (dict(dims=(2 ** 31 - 1, 1, 1)), "too large"),
        (dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "too large"),
        (dict(lo=(0.0, nan, 0.0)), "finite"), (dict(lo=(inf, 0.0, 0.0)), "finite"), (dict(step=(0.1, 0.1, -inf)), "finite"), (dict(step=(nan, 0.1, 0.1)), "finite"),
        (dict(thr=-1e-30), "threshold"), (dict(thr=nan), "threshold"), (dict(thr=-inf), "threshold"),
        (dict(sigma=False, bits=False), "at least one"),
        (dict(bits=False, count=True), "need occ_bits"), (dict(bits=False, bounds=True), "need occ_bits"),
    ]
    for kw, text in cases:
        rc, msg = _grid(L, device, **kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    # nothing wrong but the context: the last check that needs no device
    for kw in (dict(), dict(step=(0.0, -0.5, 0.1)), dict(thr=inf), dict(thr=-5.0, bits=False), dict(sigma=False, count=True, bounds=True)):
        rc, msg = _grid(L, device, **kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)


def test_batch_argument_errors_need_no_device(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    pts = np.zeros((3, 4), np.float32); sig = np.zeros(4, np.float32)
    p, s = pts.ctypes.data_as(_lib.f32p), sig.ctypes.data_as(_lib.f32p)
    for which in (-1, 2):
        assert L.nerf_density_batch(None, which, p, 4, s) == INVALID and b"which" in L.nerf_last_error(None)
        assert L.nerf_density_batch_device(None, which, pts.ctypes.data, 4, sig.ctypes.data, None) == INVALID and b"which" in L.nerf_last_error(None)
    for n in (0, 4):                                           # without a context even the empty batch is an error, not a crash
        assert L.nerf_density_batch(None, 0, p, n, s) == INVALID and L.nerf_last_error(None) == b"ctx is NULL"
        assert L.nerf_density_batch_device(None, 1, pts.ctypes.data, n, sig.ctypes.data, None) == INVALID and L.nerf_last_error(None) == b"ctx is NULL"


def test_python_layer_checks_shapes_without_a_device(native):
    net = native.Network(renderer=None, which=1)                # never reaches the library
    with pytest.raises(native.NerfError):
        net.density(np.zeros((4, 3), np.float32))
    with pytest.raises(native.NerfError):
        net.density_grid((0, 0), (1, 1, 1), (2, 2, 2))
    with pytest.raises(native.NerfError):
        net.density_grid((0, 0, 0), (1, 1, 1), (2, 2.5, 2))
    with pytest.raises(native.NerfError):
        net.density_grid((0, 0, 0), (1, 1, 1), (2, 2))


def test_unpack_occupancy_against_hand_written_words(native):
    # 5 x 3 x 2 = 30 cells in one word: cells 0, 4 (end of the first x row), 5 (start of the second), 14, 15 (first of z = 1), 29 (the last)
    word = (1 << 0) | (1 << 4) | (1 << 5) | (1 << 14) | (1 << 15) | (1 << 29)
    occ = native.unpack_occupancy(np.array([word], np.uint32), (5, 3, 2))
    assert occ.shape == (2, 3, 5) and occ.dtype == bool
    want = np.zeros((2, 3, 5), bool)
    for iz, iy, ix in ((0, 0, 0), (0, 0, 4), (0, 1, 0), (0, 2, 4), (1, 0, 0), (1, 2, 4)):
        want[iz, iy, ix] = True
    assert np.array_equal(occ, want)
    # 33 x 2 x 1 = 66 cells in three words: cell 31 (last bit of word 0), 32 (first of word 1, still row 0), 33 (first of row 1), 65 (bit 1 of word 2)
    words = np.array([1 << 31, 0b11, 0b10], np.uint32)
    occ = native.unpack_occupancy(words, (33, 2, 1))
    assert occ.shape == (1, 2, 33) and sorted(zip(*np.nonzero(occ))) == [(0, 0, 31), (0, 0, 32), (0, 1, 0), (0, 1, 32)]
    assert not native.unpack_occupancy(np.zeros(1, np.uint32), (1, 1, 1)).any()
    assert native.unpack_occupancy(np.array([1], np.uint32), (1, 1, 1)).all()
    assert native.unpack_occupancy(words.astype(">u4"), (33, 2, 1)).sum() == 4        # values, not bytes: any integer dtype
    for bad_bits, dims in ((words[:2], (33, 2, 1)), (words, (32, 2, 1)), (words, (0, 2, 1))):
        with pytest.raises(native.NerfError):
            native.unpack_occupancy(bad_bits, dims)
