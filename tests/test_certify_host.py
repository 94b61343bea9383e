"""certify_zero's stage entry points, host side (no device): the four functions exist with the ctypes signatures, and every argument error
the header lists is refused before anything touches a device -- the checks that need no context come first, so they can be told apart by their
messages even with a NULL context."""
import ctypes as C

import numpy as np

INVALID = -1
G = 64   # NERF_STAGE_GUARD_WORDS


def test_symbols_and_signatures(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    f32p, u32p, i32p, vp, u32, ci, cf, sz = _lib.f32p, _lib.u32p, _lib.i32p, C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_size_t
    want = {
        "nerf_stage_cert_plan": [vp, sz, ci, cf, cf, cf, u32, u32, u32, ci, cf, u32, u32, f32p, f32p, i32p, u32p, u32p, u32p, i32p],
        "nerf_stage_cert_verify": [vp, sz, ci, cf, u32, f32p, i32p, f32p, u32p, u32p, u32p],
        "nerf_stage_cert_audit": [vp, u32p, u32, u32, sz, f32p, u32p],
        "nerf_stage_prefilter": [vp, ci, ci, f32p, f32p, f32p, sz, ci, cf, cf, f32p, u32p],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        res, proto = _lib.PROTOTYPES[name]
        assert res is C.c_int and proto == args, name
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    for name in ("stage_cert_plan", "stage_cert_verify", "stage_cert_audit", "stage_prefilter"):
        assert callable(getattr(native.Renderer, name)), name
    assert native.api.STAGE_GUARD_WORDS == G


def _plan(L, n_rays=2, spr=8, margin=0.5, depth=9.6, mask=127, near=15, back=1, zt=0.05, cap=16, acap=16, null=None):
    from nerf_rs_amd import _lib
    t = np.zeros(16, np.float32); pre = np.zeros(16, np.float32); js = np.zeros(4, np.int32)
    lst = np.zeros(16 + 2 * G, np.uint32); cnt = np.zeros(3, np.uint32); aux = np.zeros(32 + 2 * G, np.uint32); rpw = np.zeros(1, np.int32)
    ptr = dict(t=t.ctypes.data_as(_lib.f32p), pre=pre.ctypes.data_as(_lib.f32p), js=js.ctypes.data_as(_lib.i32p), lst=lst.ctypes.data_as(_lib.u32p),
               cnt=cnt.ctypes.data_as(_lib.u32p), aux=aux.ctypes.data_as(_lib.u32p))
    if null:
        ptr[null] = None
    rc = L.nerf_stage_cert_plan(None, n_rays, spr, 6.0, margin, depth, mask, near, 0, back, zt, cap, acap, ptr["t"], ptr["pre"], ptr["js"], ptr["lst"],
                                ptr["cnt"], ptr["aux"], rpw.ctypes.data_as(_lib.i32p))
    return rc, L.nerf_last_error(None).decode()


def test_plan_argument_errors_need_no_device(native):
    L = native.load_library()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(spr=0), "spr must be positive"), (dict(spr=-3), "spr must be positive"), (dict(spr=9665), "too many samples per ray"),
             (dict(n_rays=2 ** 31, spr=8), "31 index bits"), (dict(n_rays=2 ** 28 + 1, spr=8), "31 index bits"),
             (dict(cap=17), "list_capacity exceeds"), (dict(acap=17), "aux_capacity exceeds"),
             (dict(margin=nan), "margin"), (dict(margin=-0.5), "margin"), (dict(margin=inf), "margin"),
             (dict(zt=nan), "zero_threshold"), (dict(depth=nan), "depth_limit"),
             (dict(mask=126), "2^k - 1"), (dict(near=5), "2^k - 1")] + [(dict(null=k), "NULL buffer") for k in ("t", "pre", "js", "lst", "cnt", "aux")]
    for kw, text in cases:
        rc, msg = _plan(L, **kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    # nothing wrong but the context: the last check that needs no device (rays_per_wave_out may be NULL; a NaN threshold is ignored without a back part)
    for kw in (dict(), dict(spr=9664, n_rays=0, cap=0, acap=0), dict(back=0, zt=nan), dict(margin=0.0), dict(mask=0, near=0xFFFFFFFF), dict(cap=0, acap=0), dict(depth=-inf)):
        rc, msg = _plan(L, **kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)


def test_verify_argument_errors_need_no_device(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    t = np.zeros(16, np.float32); s = np.zeros(16, np.float32); lst = np.zeros(16 + 2 * G, np.uint32)
    cnt = np.zeros(1, np.uint32); fb = np.zeros(1, np.uint32)

    def call(n_rays=2, spr=8, cap=16, js=(0, 8), null=None):
        j = np.array(js, np.int32)
        ptr = dict(t=t.ctypes.data_as(_lib.f32p), j=j.ctypes.data_as(_lib.i32p), s=s.ctypes.data_as(_lib.f32p), lst=lst.ctypes.data_as(_lib.u32p),
                   cnt=cnt.ctypes.data_as(_lib.u32p), fb=fb.ctypes.data_as(_lib.u32p))
        if null:
            ptr[null] = None
        rc = L.nerf_stage_cert_verify(None, n_rays, spr, 6.0, cap, ptr["t"], ptr["j"], ptr["s"], ptr["lst"], ptr["cnt"], ptr["fb"])
        return rc, L.nerf_last_error(None).decode()

    cases = [(dict(spr=0), "spr must be positive"), (dict(spr=10241), "too many samples per ray"), (dict(n_rays=2 ** 31), "31 index bits"),
             (dict(cap=17), "list_capacity exceeds"), (dict(js=(0, 9)), "jstar must lie in"), (dict(js=(-1, 3)), "jstar must lie in")]
    cases += [(dict(null=k), "NULL buffer") for k in ("t", "j", "s", "lst", "cnt", "fb")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    for kw in (dict(), dict(cap=0), dict(js=(8, 8))):
        rc, msg = call(**kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)


def test_audit_argument_errors_need_no_device(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    aux = np.array([[0, 0], [3, 0], [9, 0]], np.uint32); s = np.zeros(8, np.float32); w = np.zeros(4, np.uint32)
    a, sp, wp = aux.ctypes.data_as(_lib.u32p), s.ctypes.data_as(_lib.f32p), w.ctypes.data_as(_lib.u32p)

    def call(*args):
        return L.nerf_stage_cert_audit(None, *args), L.nerf_last_error(None).decode()

    for args, text in (((a, 3, 3, 8, sp, wp), "outside sigma"), ((a, 2, 3, 2 ** 31, sp, wp), "31 index bits"), ((a, 2, 3, 8, sp, None), "NULL buffer"),
                       ((None, 2, 3, 8, sp, wp), "NULL buffer"), ((a, 2, 3, 8, None, wp), "NULL buffer")):
        rc, msg = call(*args)
        assert rc == INVALID and text in msg, (args[1:4], rc, msg)
    # the record outside sigma lies beyond min(aux_count, aux_capacity): not looked at; no records: no buffers needed
    for args in ((a, 2, 3, 8, sp, wp), (a, 3, 2, 8, sp, wp), (None, 0, 5, 0, None, wp), (None, 7, 0, 0, None, wp)):
        rc, msg = call(*args)
        assert rc == INVALID and msg == "ctx is NULL", (args[1:4], rc, msg)


def test_prefilter_argument_errors_need_no_device(native):
    from nerf_rs_amd import _lib
    L = native.load_library()
    o = np.zeros(3, np.float32); d = np.zeros(6, np.float32); t = np.zeros(16, np.float32); out = np.zeros(16, np.float32); bad = np.zeros(1, np.uint32)
    P = lambda x: x.ctypes.data_as(_lib.f32p)

    def call(which=0, f16=1, n_rays=2, spr=8, cut=0.0, null=None):
        ptr = dict(o=P(o), d=P(d), t=P(t), out=P(out), bad=bad.ctypes.data_as(_lib.u32p))
        if null:
            ptr[null] = None
        rc = L.nerf_stage_prefilter(None, which, f16, ptr["o"], ptr["d"], ptr["t"], n_rays, spr, 6.0, cut, ptr["out"], ptr["bad"])
        return rc, L.nerf_last_error(None).decode()

    cases = [(dict(which=2), "which"), (dict(which=-1), "which"), (dict(spr=0), "spr must be positive"), (dict(n_rays=2 ** 31), "too many samples"),
             (dict(cut=-0.1), "cut_T"), (dict(cut=1.0), "cut_T"), (dict(cut=float("nan")), "cut_T")]
    cases += [(dict(null=k), "NULL buffer") for k in ("o", "d", "t", "out", "bad")]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == INVALID and text in msg, (kw, rc, msg)
    for kw in (dict(), dict(f16=0, which=1, cut=4.1e-5), dict(n_rays=0)):
        rc, msg = call(**kw)
        assert rc == INVALID and msg == "ctx is NULL", (kw, rc, msg)
