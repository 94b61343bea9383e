"""Host-side mirror of the reference's interface for the hot path, over the C ABI.

Reference names kept (elisabeth96/nerf-rs):
  load_network_from_dir   src/lib.rs:108-174
  Network.forward_batch   src/network.rs:197-237   (points 3 x B SoA, view_dirs B x 3 -> colours B x 3, sigma B)
  Camera / camera_from_samples   src/lib.rs:197-211, 614-645
  render_image            src/lib.rs:474-565      (-> ny x nx x 3 linear RGB, pixel (i, j) at [i, j])
  save_ppm                src/lib.rs:567-580
Errors the reference raises as panics surface as NerfError with the same message text.
"""
import collections
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import CCamera, CComponent, CComponentFilter, COpts, CStats, NerfError, check, f32p, i32p, u8p, u32p

NET_COARSE, NET_FINE = 0, 1
MLP_F32, MLP_BF16 = 0, 1
ALPHA_OPAQUE, ALPHA_PREMULTIPLIED, ALPHA_STRAIGHT = 0, 1, 2
STAGE_GUARD_WORDS = 64  # NERF_STAGE_GUARD_WORDS
_ALPHAS = {"opaque": 0, "premultiplied": 1, "straight": 2}
_DTYPES = {"f32": 0, "float32": 0, 0: 0, "bf16": 1, "bfloat16": 1, 1: 1, "bf16x3": 2, 2: 2, "f16x2": 3, 3: 3}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(f32p)


def _background(background):
    """None (white, the reference) or three floats -> what the C ABI takes (the array must outlive the call)."""
    if background is None:
        return None, None
    b = _f32(background).reshape(-1)
    if b.size != 3:
        raise NerfError(-1, "background must be None or three floats (R, G, B)")
    return b, _p(b)


def _alpha(alpha):
    """'opaque' | 'premultiplied' | 'straight' or the NERF_ALPHA_* number (the library rejects a number out of range)."""
    if isinstance(alpha, str):
        if alpha not in _ALPHAS:
            raise NerfError(-1, "alpha must be 'opaque', 'premultiplied' or 'straight'")
        return _ALPHAS[alpha]
    return int(alpha)


class Stats:
    def __init__(self, c):
        for name, _ in CStats._fields_:
            v = getattr(c, name)
            setattr(self, name, v if isinstance(v, (int, float)) else tuple(v))

    def __repr__(self):
        return "Stats(" + ", ".join(f"{k}={v}" for k, v in self.__dict__.items()) + ")"


class Renderer:
    """One context = one GPU (nerf_create).  Holds the two networks the way render_cli_image does (src/lib.rs:651-652)."""

    def __init__(self, device=0):
        self._L = _lib.load_library()
        h = C.c_void_p()
        check(self._L.nerf_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self.coarse = None
        self.fine = None

    def close(self):
        if getattr(self, "handle", None):
            self._L.nerf_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        n = C.c_int()
        buf = C.create_string_buffer(64)
        check(self._L.nerf_device_info(self.handle, C.byref(n), buf, 64), self.handle)
        return {"n_cus": n.value, "arch": buf.value.decode()}

    def load_scene(self, root):
        """lego_rust/{coarse,fine} (src/lib.rs:650-652)."""
        import os
        self.coarse = load_network_from_dir(self, NET_COARSE, os.path.join(root, "coarse"))
        self.fine = load_network_from_dir(self, NET_FINE, os.path.join(root, "fine"))
        return self.coarse, self.fine

    def kernel_time_query(self, reset=True):
        ms, pts, n = C.c_double(), C.c_uint64(), C.c_uint32()
        check(self._L.nerf_kernel_time_query(self.handle, C.byref(ms), C.byref(pts), C.byref(n), int(reset)), self.handle)
        return ms.value, pts.value, n.value

    def workgroup_clocks(self):
        """Per persistent workgroup {shader cycles, 100 MHz ticks} of the last fine (NERF_DEBUG_CLOCK=1) or sampling (=2) launch -> (n_cus, 2) uint64."""
        out = np.zeros((self.device_info()["n_cus"], 2), np.uint64)
        check(self._L.nerf_debug_workgroup_clocks(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.shape[0]), self.handle)
        return out

    # ---- stage entry points (parity tests; hosts that own ray setup) ----
    def stage_ray_dirs(self, cam, x0, y0, w, h, normalize=True):
        out = np.empty((h, w, 3), np.float32)
        check(self._L.nerf_stage_ray_dirs(self.handle, C.byref(cam.c), x0, y0, w, h, int(normalize), _p(out)), self.handle)
        return out

    def stage_stratified(self, cam, x0, y0, w, h, count, seed=0):
        out = np.empty((h, w, count), np.float32)
        check(self._L.nerf_stage_stratified(self.handle, C.byref(cam.c), x0, y0, w, h, count, seed, _p(out)), self.handle)
        return out

    def stage_resample(self, t_coarse, sigma_coarse, nf, far, seed=0, pixel_index=None, u=None):
        t = _f32(t_coarse); s = _f32(sigma_coarse)
        R, nc = t.shape
        w = np.empty((R, nc), np.float32); cdf = np.empty((R, nc - 1), np.float32)
        tn = np.empty((R, nf), np.float32); tf = np.empty((R, nc + nf), np.float32)
        pix = None if pixel_index is None else np.ascontiguousarray(pixel_index, dtype=np.uint32)
        uu = None if u is None else _f32(u)
        check(self._L.nerf_stage_resample(self.handle, R, nc, nf, far, seed,
                                          None if pix is None else pix.ctypes.data_as(u32p), _p(t), _p(s),
                                          None if uu is None else _p(uu), _p(w), _p(cdf), _p(tn), _p(tf)), self.handle)
        return {"w": w, "cdf": cdf, "t_new": tn, "t_fine": tf}

    def stage_depth_order(self, t):
        """The depth-order table of an image pass with sample positions t (rows, rays_per_row, samples_per_ray): the slots of the first
        (rows // 4) * 4 rows, per 8 x 4 pixel block in ascending (bits of t, ray-in-block, sample) order (nerf_stage_depth_order) -> uint32."""
        t = _f32(t)
        rows, rw, spr = t.shape
        out = np.empty((rows // 4) * 4 * rw * spr, np.uint32)
        check(self._L.nerf_stage_depth_order(self.handle, rows, rw, spr, _p(t), out.ctypes.data_as(u32p)), self.handle)
        return out

    def stage_depth_order_flags(self, t):
        """The order kernel's word per 8 x 4 pixel block of the same pass: 1 where every ray's samples stand in the table in sample-index order
        (the keys of each of the block's rows ascend), else 0 (nerf_stage_depth_order_flags) -> uint32 ((rows // 4) * (rays_per_row // 8),)."""
        t = _f32(t)
        rows, rw, spr = t.shape
        out = np.empty((rows // 4) * (rw // 8), np.uint32)
        check(self._L.nerf_stage_depth_order_flags(self.handle, rows, rw, spr, _p(t), out.ctypes.data_as(u32p)), self.handle)
        return out

    def stage_hybrid_flags(self, t_coarse, sigma_coarse, nf, far, seed=0, pixel_index=None, u=None, tau=0.0):
        """hybrid_sampling's per-ray decision for the given coarse densities -> (flags (R,) bool, t_new (R, nf) unsorted draws)."""
        t = _f32(t_coarse); s = _f32(sigma_coarse)
        R, nc = t.shape
        flags = np.zeros(R, np.uint8); tn = np.empty((R, nf), np.float32)
        pix = None if pixel_index is None else np.ascontiguousarray(pixel_index, dtype=np.uint32)
        uu = None if u is None else _f32(u)
        check(self._L.nerf_stage_hybrid_flags(self.handle, R, nc, nf, far, seed, None if pix is None else pix.ctypes.data_as(u32p),
                                              _p(t), _p(s), None if uu is None else _p(uu), tau,
                                              flags.ctypes.data_as(C.POINTER(C.c_uint8)), _p(tn)), self.handle)
        return flags.astype(bool), tn

    def stage_integrate(self, rgb, sigma, t, far):
        c = _f32(rgb); s = _f32(sigma); t = _f32(t)
        R, n = t.shape
        out = np.empty((R, 3), np.float32); w = np.empty((R, n), np.float32)
        check(self._L.nerf_stage_integrate(self.handle, R, n, far, _p(c), _p(s), _p(t), _p(out), _p(w)), self.handle)
        return out, w

    def stage_ray_quantiles(self, w, t, quantiles):
        """The quantile walk on caller data (nerf_stage_ray_quantiles): w, t (R, n) -> depth_q (n_q, R)."""
        ww = _f32(w); tt = _f32(t)
        if ww.ndim != 2 or ww.shape != tt.shape:
            raise NerfError(-1, "w and t must be (n_rays, n) arrays of one shape")
        qs = _quantile_args(quantiles)
        R, n = tt.shape
        out = np.empty((qs.size, R), np.float32)
        check(self._L.nerf_stage_ray_quantiles(self.handle, R, n, _p(ww), _p(tt), _p(qs), qs.size, _p(out)), self.handle)
        return out

    def stage_gather_points(self, origins, dirs, depth_q, rgb, opacity, normals=None, min_opacity=0.5, capacity=None):
        """The point compaction on caller data (nerf_stage_gather_points) -> a dict: n_points (the full count), overflow (True when it
        exceeds the capacity: the library's NERF_ERR_STATE), xyz, rgb, [normals,] ray, depth, opacity -- each the `capacity` records as
        the device held them (0xFFFFFFFF words = never written) -- and guards = the words behind every array."""
        o, d, _, n = _ray_args(origins, dirs, None)
        dq, c, a = _f32(depth_q), _f32(rgb), _f32(opacity)
        nr = None if normals is None else _f32(normals)
        if dq.shape != (n,) or a.shape != (n,) or c.shape != (n, 3) or (nr is not None and nr.shape != (n, 3)):
            raise NerfError(-1, "depth_q and opacity must be (n,) arrays, rgb and normals (n, 3)")
        cap = n if capacity is None else int(capacity)
        if cap < 0:
            raise NerfError(-1, "capacity must not be negative")
        G = 64  # NERF_STAGE_GUARD_WORDS
        bufs = {k: np.zeros(w * cap + G, np.uint32) for k, w in (("xyz", 3), ("rgb", 3), ("normals", 3), ("ray", 1), ("depth", 1), ("opacity", 1))
                if k != "normals" or nr is not None}
        cnt = C.c_size_t(0)
        code = self._L.nerf_stage_gather_points(self.handle, n, _p(o), 1 if o.ndim == 1 else n, _p(d), _p(dq), _p(c), _p(a),
                                                None if nr is None else _p(nr), float(min_opacity), cap,
                                                bufs["xyz"].ctypes.data_as(f32p), bufs["rgb"].ctypes.data_as(f32p),
                                                bufs["normals"].ctypes.data_as(f32p) if nr is not None else None, bufs["ray"].ctypes.data_as(u32p),
                                                bufs["depth"].ctypes.data_as(f32p), bufs["opacity"].ctypes.data_as(f32p), C.byref(cnt))
        if code != 0 and not (code == -6 and cnt.value > cap):
            check(code, self.handle)
        out = {"n_points": int(cnt.value), "overflow": code != 0, "guards": {k: v[len(v) - G:].copy() for k, v in bufs.items()}}
        for k, v in bufs.items():
            body = v[:len(v) - G]
            out[k] = body.copy() if k == "ray" else body.view(np.float32).reshape((cap, 3) if k in ("xyz", "rgb", "normals") else (cap,)).copy()
        return out

    def stage_integrate_rgba8(self, rgb, sigma, t, far, background=None, alpha="opaque"):
        """integrate_ray + the RGBA8 pack (nerf_stage_integrate_rgba8) -> (R, 4) uint8."""
        c = _f32(rgb); s = _f32(sigma); t = _f32(t)
        R, n = t.shape
        out = np.empty((R, 4), np.uint8)
        keep, bg = _background(background)
        check(self._L.nerf_stage_integrate_rgba8(self.handle, R, n, far, _p(c), _p(s), _p(t), bg, _alpha(alpha),
                                                 out.ctypes.data_as(u8p)), self.handle)
        return out

    # ---- certify_zero's device pieces, one launch each (include/nerf_mi355x.h) ----
    def stage_cert_plan(self, pre, t, far, margin, depth_limit, audit_mask=127, audit_mask_near=15, audit_salt=0, zero_threshold=None,
                        list_capacity=None, aux_capacity=None):
        """k_cert_plan on (R, spr) pre-activations; zero_threshold=None: no back part.  Returns a dict: pre (rewritten), jstar, list (the
        capacity entries, 0xFFFFFFFF = never written), counts (front, back, aux), aux ((aux_capacity, 2) records), rays_per_wave, and
        guards = the guard words around list and aux (all still 0xFFFFFFFF unless the kernel wrote out of bounds)."""
        p = _f32(pre).copy(); tt = _f32(t)
        R, spr = p.shape
        cap = R * spr if list_capacity is None else int(list_capacity)
        acap = R * spr if aux_capacity is None else int(aux_capacity)
        G = STAGE_GUARD_WORDS
        lst = np.zeros(cap + 2 * G, np.uint32); aux = np.zeros(2 * acap + 2 * G, np.uint32)
        js = np.zeros(R, np.int32); cnt = np.zeros(3, np.uint32); rpw = np.zeros(1, np.int32)
        check(self._L.nerf_stage_cert_plan(self.handle, R, spr, far, margin, depth_limit, audit_mask, audit_mask_near, audit_salt,
                                           int(zero_threshold is not None), 0.0 if zero_threshold is None else zero_threshold, cap, acap,
                                           _p(tt), _p(p), js.ctypes.data_as(i32p), lst.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p),
                                           aux.ctypes.data_as(u32p), rpw.ctypes.data_as(i32p)), self.handle)
        return {"pre": p, "jstar": js, "list": lst[G:G + cap], "counts": tuple(int(x) for x in cnt), "aux": aux[G:G + 2 * acap].reshape(acap, 2),
                "rays_per_wave": int(rpw[0]), "guards": np.concatenate([lst[:G], lst[G + cap:], aux[:G], aux[G + 2 * acap:]])}

    def stage_cert_verify(self, sigma, t, far, jstar, list_capacity=None, count=0, fallback_rays=0):
        """k_cert_verify on (R, spr) exact densities with marks (-1) -> dict: sigma, list, count, fallback_rays, guards."""
        s = _f32(sigma).copy(); tt = _f32(t)
        R, spr = s.shape
        cap = R * spr if list_capacity is None else int(list_capacity)
        G = STAGE_GUARD_WORDS
        js = np.ascontiguousarray(jstar, dtype=np.int32)
        lst = np.zeros(cap + 2 * G, np.uint32); cnt = np.array([count], np.uint32); fb = np.array([fallback_rays], np.uint32)
        check(self._L.nerf_stage_cert_verify(self.handle, R, spr, far, cap, _p(tt), js.ctypes.data_as(i32p), _p(s), lst.ctypes.data_as(u32p),
                                             cnt.ctypes.data_as(u32p), fb.ctypes.data_as(u32p)), self.handle)
        return {"sigma": s, "list": lst[G:G + cap], "count": int(cnt[0]), "fallback_rays": int(fb[0]),
                "guards": np.concatenate([lst[:G], lst[G + cap:]])}

    def stage_cert_audit(self, aux, sigma, audit=(0, 0, 0, 0), aux_count=None, aux_capacity=None):
        """k_cert_audit on (n, 2) uint32 records and the flat density buffer -> (sigma, the four audit words)."""
        a = np.ascontiguousarray(aux, dtype=np.uint32).reshape(-1, 2)
        s = _f32(sigma).reshape(-1).copy()
        w = np.array(audit, np.uint32)
        n = len(a) if aux_count is None else int(aux_count)
        cap = len(a) if aux_capacity is None else int(aux_capacity)
        check(self._L.nerf_stage_cert_audit(self.handle, a.ctypes.data_as(u32p), n, cap, s.size, _p(s), w.ctypes.data_as(u32p)), self.handle)
        return s, w

    def stage_prefilter(self, which, origin, dirs, t, far, f16=True, cut_T=0.0, origins=None):
        """The ray-sequential 16-bit pre-filter of network `which` -> (raw pre-activations (R, spr), non-finite tile count).
        origins (R, 3) in place of origin (then None): one origin per ray (nerf_stage_prefilter_rays)."""
        d = _f32(dirs).reshape(-1, 3); tt = _f32(t)
        R, spr = tt.shape
        if len(d) != R:
            raise NerfError(-1, "dirs must hold one direction per ray")
        if (origin is None) == (origins is None):
            raise NerfError(-1, "give either origin or origins")
        o = _f32(origin).reshape(3) if origins is None else _f32(origins).reshape(-1, 3)
        if origins is not None and len(o) != R:
            raise NerfError(-1, "origins must hold one origin per ray")
        out = np.empty((R, spr), np.float32); bad = np.zeros(1, np.uint32)
        call = self._L.nerf_stage_prefilter if origins is None else self._L.nerf_stage_prefilter_rays
        check(call(self.handle, int(which), int(bool(f16)), _p(o), _p(d), _p(tt), R, spr, far, cut_T, _p(out), bad.ctypes.data_as(u32p)), self.handle)
        return out, int(bad[0])


class Network:
    """network::Network (src/network.rs:172-238) resident on the GPU."""

    def __init__(self, renderer, which):
        self.renderer = renderer
        self.which = which

    def forward_batch(self, points, view_dirs, dtype="f32"):
        """points: (3, B) f32 SoA; view_dirs: (B, 3) -> (colours (B, 3), sigma (B,)).  B == 0 returns empties
        (src/network.rs:199-201)."""
        pts = _f32(points); dirs = _f32(view_dirs)
        if pts.ndim != 2 or pts.shape[0] != 3:
            raise NerfError(-1, "points must be a 3 x B matrix")  # debug_assert_eq!(points.rows(), 3)
        n = pts.shape[1]
        if dirs.shape != (n, 3):
            raise NerfError(-1, "view_dirs must have one direction per column")  # debug_assert_eq!(batch, view_dirs.len())
        rgb = np.empty((n, 3), np.float32); sig = np.empty((n,), np.float32)
        if n:
            R = self.renderer
            check(R._L.nerf_forward_batch_ex(R.handle, self.which, _DTYPES[dtype], _p(pts), _p(dirs), n, _p(rgb), _p(sig)), R.handle)
        return rgb, sig

    def forward_batch_device(self, d_points, d_view_dirs, d_rgb, d_sigma, n, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`."""
        R = self.renderer
        check(R._L.nerf_forward_batch_device(R.handle, self.which, d_points, d_view_dirs, n, d_rgb, d_sigma, stream), R.handle)

    def density(self, points):
        """sigma alone at points (3, B) f32 SoA -> (B,): the bits forward_batch returns as sigma, without directions and without the
        colour head (nerf_density_batch; f32 arithmetic).  B == 0 returns an empty array."""
        pts = _f32(points)
        if pts.ndim != 2 or pts.shape[0] != 3:
            raise NerfError(-1, "points must be a 3 x B matrix")
        n = pts.shape[1]
        sig = np.empty((n,), np.float32)
        if n:
            R = self.renderer
            check(R._L.nerf_density_batch(R.handle, self.which, _p(pts), n, _p(sig)), R.handle)
        return sig

    def density_device(self, d_points, d_sigma, n, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`."""
        R = self.renderer
        check(R._L.nerf_density_batch_device(R.handle, self.which, d_points, n, d_sigma, stream), R.handle)

    def density_gradient(self, points, h):
        """Central differences of sigma at points (3, B) f32 SoA with step h (finite, > 0) -> (3, B): per axis
        (sigma(p + h e) - sigma(p - h e)) / (fl(p + h) - fl(p - h)) in f32, each operation rounded once, 0 where the denominator is 0
        (nerf_density_gradient_batch; the sigmas are density()'s bits).  B == 0 returns an empty array."""
        pts = _f32(points)
        if pts.ndim != 2 or pts.shape[0] != 3:
            raise NerfError(-1, "points must be a 3 x B matrix")
        n = pts.shape[1]
        grad = np.empty((3, n), np.float32)
        R = self.renderer
        check(R._L.nerf_density_gradient_batch(R.handle, self.which, _p(pts), n, float(h), _p(grad)), R.handle)
        return grad

    def density_gradient_device(self, d_points, d_grad, n, h, stream=0):
        """Raw device pointers (ints), asynchronous on `stream`."""
        R = self.renderer
        check(R._L.nerf_density_gradient_batch_device(R.handle, self.which, d_points, n, float(h), d_grad, stream), R.handle)

    def density_grid(self, lo, step, dims, threshold=None, want_sigma=True):
        """sigma on the lattice lo + step * (ix, iy, iz), 0 <= i* < dims = (nx, ny, nz), generated inside the kernel (nerf_density_grid)
        -> (sigma, bits, count, bounds): sigma (nz, ny, nx) f32 or None (want_sigma=False); with a threshold (>= 0) bits = ceil(N / 32)
        uint32 words, bit b of word w = sigma of linear cell 32 w + b > threshold (see unpack_occupancy), count = number of occupied cells,
        bounds = (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max), inclusive -- dims and (-1, -1, -1) if no cell is occupied; without a
        threshold bits, count and bounds are None."""
        lo_c, step_c, dims_c, n = _grid_args(lo, step, dims)
        nx, ny, nz = (int(v) for v in dims_c)
        sig = np.empty((nz, ny, nx), np.float32) if want_sigma and n > 0 else None
        bits = np.empty(((n + 31) // 32,), np.uint32) if threshold is not None and n > 0 else None
        cnt, bounds = C.c_uint64(0), np.zeros(6, np.int32)
        R = self.renderer
        check(R._L.nerf_density_grid(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p),
                                     None if sig is None else _p(sig), 0.0 if threshold is None else float(threshold),
                                     None if bits is None else bits.ctypes.data_as(u32p),
                                     None if bits is None else C.byref(cnt), None if bits is None else bounds.ctypes.data_as(i32p)), R.handle)
        if bits is None:
            return sig, None, None, None
        return sig, bits, int(cnt.value), tuple(int(v) for v in bounds)

    def density_grid_device(self, lo, step, dims, d_sigma=None, threshold=0.0, d_bits=None, want_stats=False, stream=0):
        """Raw device pointers (ints; either may be None): d_sigma nz * ny * nx floats, d_bits ceil(N / 32) words.  Asynchronous on `stream`;
        want_stats (needs d_bits) synchronises it and returns (count, bounds), else None."""
        lo_c, step_c, dims_c, _ = _grid_args(lo, step, dims)
        cnt, bounds = C.c_uint64(0), np.zeros(6, np.int32)
        R = self.renderer
        check(R._L.nerf_density_grid_device(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), d_sigma, float(threshold),
                                            d_bits, C.byref(cnt) if want_stats else None,
                                            bounds.ctypes.data_as(i32p) if want_stats else None, stream), R.handle)
        return (int(cnt.value), tuple(int(v) for v in bounds)) if want_stats else None


    def extract_mesh(self, lo, step, dims, iso, normals=False, colours=False, capacity=None, keep_largest=0, min_points=0, return_counts=False):
        """The level set sigma = iso of this network on the lattice lo + step * index (density_grid's lattice, every dims >= 2, no zero
        step), extracted on the device by marching tetrahedra (nerf_extract_mesh; conventions: include/nerf_mi355x.h) -> Mesh(vertices
        (V, 3) f32, normals (V, 3) f32 or None, colours (V, 3) f32 or None, triangles (T, 3) uint32).  The sigma lattice never reaches
        the host.  normals: unit vectors towards lower density; colours: the network's rgb at the vertices seen head-on (dirs = -normal).

        capacity=None asks the library for the counts first and then calls it again with arrays of that size: A QUERY FOLLOWED BY A FILL
        EVALUATES THE LATTICE TWICE (the network launch included).  capacity=(max_vertices, max_triangles) is one call; a mesh that
        does not fit raises NerfError with the counts in the message (nothing was written).

        keep_largest / min_points (nerf_extract_mesh_filtered; "lattice components" in the header): only the components of the inside points
        (14-neighbour Kuhn connectivity) with at least min_points lattice points and, if keep_largest > 0, among the keep_largest largest
        (ties: smaller label first) are meshed -- keep_largest=1 drops every floater.  Both 0 (the default): the unfiltered entry point.
        return_counts=True -> (Mesh, n_components, n_kept)."""
        lo_c, step_c, dims_c, _ = _grid_args(lo, step, dims)
        R = self.renderer
        filt, nc, nk = _filter_args(keep_largest, min_points, return_counts)
        if filt is None and not return_counts:
            call = lambda v, n, c, cv, t, ct, nv, nt: R._L.nerf_extract_mesh(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), float(iso),
                                                                             v, n, c, cv, t, ct, nv, nt)
        else:
            call = lambda v, n, c, cv, t, ct, nv, nt: R._L.nerf_extract_mesh_filtered(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p),
                                                                                      float(iso), None if filt is None else C.addressof(filt),
                                                                                      v, n, c, cv, t, ct, nv, nt, C.byref(nc) if return_counts else None,
                                                                                      C.byref(nk) if return_counts else None)
        mesh = _mesh_call(call, R.handle, bool(normals), bool(colours), capacity)
        return (mesh, int(nc.value), int(nk.value)) if return_counts else mesh

    def extract_mesh_device(self, lo, step, dims, iso, d_vertices, d_normals, d_colours, cap_vertices, d_triangles, cap_triangles, stream=0,
                            keep_largest=0, min_points=0, return_counts=False):
        """Raw device pointers (ints; each may be None) -> (n_vertices, n_triangles).  Synchronises `stream` to read the counts; the arrays are
        written (asynchronously) only if both counts fit the capacities.  keep_largest / min_points as in extract_mesh
        (nerf_extract_mesh_filtered_device); return_counts=True -> (n_vertices, n_triangles, n_components, n_kept)."""
        lo_c, step_c, dims_c, _ = _grid_args(lo, step, dims)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        R = self.renderer
        filt, nc, nk = _filter_args(keep_largest, min_points, return_counts)
        if filt is None and not return_counts:
            check(R._L.nerf_extract_mesh_device(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), float(iso), d_vertices, d_normals,
                                                d_colours, int(cap_vertices), d_triangles, int(cap_triangles), C.byref(nv), C.byref(nt), stream), R.handle)
            return int(nv.value), int(nt.value)
        check(R._L.nerf_extract_mesh_filtered_device(R.handle, self.which, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), float(iso),
                                                     None if filt is None else C.addressof(filt), d_vertices, d_normals, d_colours, int(cap_vertices),
                                                     d_triangles, int(cap_triangles), C.byref(nv), C.byref(nt), C.byref(nc) if return_counts else None,
                                                     C.byref(nk) if return_counts else None, stream), R.handle)
        out = (int(nv.value), int(nt.value))
        return out + (int(nc.value), int(nk.value)) if return_counts else out


Mesh = collections.namedtuple("Mesh", "vertices normals colours triangles")


def _mesh_call(call, handle, normals, colours, capacity):
    """Size query + fill (capacity None) or one call with the given capacity, around `call(vertices, normals, colours, cap_v, triangles, cap_t,
    n_vertices, n_triangles)`."""
    nv, nt = C.c_uint64(0), C.c_uint64(0)
    if capacity is None:
        check(call(None, None, None, 0, None, 0, C.byref(nv), C.byref(nt)), handle)
        cap_v, cap_t = int(nv.value), int(nt.value)
    else:
        cap_v, cap_t = (int(v) for v in capacity)
        if cap_v < 0 or cap_t < 0:
            raise NerfError(-1, "capacity must be (max_vertices, max_triangles), both >= 0")
    v = np.empty((cap_v, 3), np.float32)
    n = np.empty((cap_v, 3), np.float32) if normals else None
    c = np.empty((cap_v, 3), np.float32) if colours else None
    t = np.empty((cap_t, 3), np.uint32)
    check(call(_p(v), None if n is None else _p(n), None if c is None else _p(c), cap_v, t.ctypes.data_as(u32p), cap_t, C.byref(nv), C.byref(nt)), handle)
    n_v, n_t = int(nv.value), int(nt.value)
    if n_v > cap_v or n_t > cap_t:
        raise NerfError(-1, f"capacity too small: the mesh has {n_v} vertices and {n_t} triangles")
    return Mesh(v[:n_v], None if n is None else n[:n_v], None if c is None else c[:n_v], t[:n_t])


def _filter_args(keep_largest, min_points, return_counts):
    """(CComponentFilter or None for "keep everything", n_components, n_kept) of a filtered mesh call."""
    k, m = int(keep_largest), int(min_points)
    if not (0 <= k < 2 ** 32 and 0 <= m < 2 ** 32):
        raise NerfError(-1, "keep_largest and min_points must be non-negative 32-bit integers")
    return (CComponentFilter(k, m) if (k or m > 1) else None), C.c_uint64(0), C.c_uint64(0)     # every component has a point: min_points 1 discards nothing


def isosurface(renderer, sigma, lo, step, iso, normals=False, capacity=None, keep_largest=0, min_points=0, return_counts=False):
    """The level set sigma = iso of a caller-supplied lattice sigma[iz, iy, ix] (shape (nz, ny, nx), x fastest, at the points lo + step * index)
    by marching tetrahedra on the device (nerf_isosurface_grid; needs a Renderer, no network) -> Mesh(vertices, normals or None, None,
    triangles).  capacity as in Network.extract_mesh (None: a size query, then the fill -- the lattice is uploaded and classified twice).
    keep_largest / min_points / return_counts as in Network.extract_mesh (nerf_isosurface_grid_filtered)."""
    sig = _f32(sigma)
    if sig.ndim != 3:
        raise NerfError(-1, "sigma must be a (nz, ny, nx) array")
    lo_c, step_c, dims_c, _ = _grid_args(lo, step, sig.shape[::-1])
    filt, nc, nk = _filter_args(keep_largest, min_points, return_counts)
    if filt is None and not return_counts:
        call = lambda v, n, c, cv, t, ct, nv, nt: renderer._L.nerf_isosurface_grid(renderer.handle, _p(sig), _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p),
                                                                                   float(iso), v, n, cv, t, ct, nv, nt)
    else:
        call = lambda v, n, c, cv, t, ct, nv, nt: renderer._L.nerf_isosurface_grid_filtered(renderer.handle, _p(sig), _p(lo_c), _p(step_c),
                                                                                            dims_c.ctypes.data_as(i32p), float(iso),
                                                                                            None if filt is None else C.addressof(filt), v, n, cv, t, ct,
                                                                                            nv, nt, C.byref(nc) if return_counts else None,
                                                                                            C.byref(nk) if return_counts else None)
    mesh = _mesh_call(call, renderer.handle, bool(normals), False, capacity)
    return (mesh, int(nc.value), int(nk.value)) if return_counts else mesh


Component = collections.namedtuple("Component", "label n_points bounds")


def _components_out(table, n_components):
    return [Component(int(e.label), int(e.n_points), tuple(int(v) for v in e.bounds)) for e in table[:min(len(table), n_components)]]


def lattice_components(renderer, sigma, iso, table=16, want_labels=True):
    """The connected components of the inside points (sigma > iso; 14-neighbour Kuhn connectivity, the mesh's) of a caller-supplied lattice
    sigma[iz, iy, ix], labelled on the device (nerf_lattice_components; "lattice components" in the header) -> (labels, components,
    n_components): labels (nz, ny, nx) uint32, a component's label = the smallest linear index ix + nx (iy + ny iz) among its points,
    0xFFFFFFFF where not inside (None with want_labels=False); components = the first min(table, n_components) as Component(label, n_points,
    bounds = inclusive (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max)), largest first, ties by label; table <= 64."""
    sig = _f32(sigma)
    if sig.ndim != 3:
        raise NerfError(-1, "sigma must be a (nz, ny, nx) array")
    dims_c = np.ascontiguousarray(sig.shape[::-1], dtype=np.int32)
    cap = int(table)
    if cap < 0:
        raise NerfError(-1, "table must be >= 0")
    labels = np.empty(sig.shape, np.uint32) if want_labels else None
    entries = (CComponent * max(cap, 1))()
    n = C.c_uint64(0)
    check(renderer._L.nerf_lattice_components(renderer.handle, _p(sig), dims_c.ctypes.data_as(i32p), float(iso),
                                              None if labels is None else labels.ctypes.data_as(u32p), C.addressof(entries) if cap else None, cap,
                                              C.byref(n)), renderer.handle)
    return labels, _components_out(entries[:cap], int(n.value)), int(n.value)


def lattice_components_device(renderer, d_sigma, dims, iso, d_labels=None, table=16, stream=0):
    """The same on a lattice resident on the device (raw pointers as ints: d_sigma nz * ny * nx floats, e.g. density_grid_device's output;
    d_labels N uint32 or None) -> (components, n_components).  Synchronises `stream` (nerf_lattice_components_device)."""
    d = np.asarray(dims)
    if d.size != 3 or np.any(d != np.floor(d)) or np.any(np.abs(d) >= 2 ** 31):
        raise NerfError(-1, "dims must be three integers")
    dims_c = np.ascontiguousarray(d.reshape(-1), dtype=np.int32)
    cap = int(table)
    if cap < 0:
        raise NerfError(-1, "table must be >= 0")
    entries = (CComponent * max(cap, 1))()
    n = C.c_uint64(0)
    check(renderer._L.nerf_lattice_components_device(renderer.handle, d_sigma, dims_c.ctypes.data_as(i32p), float(iso), d_labels,
                                                     C.addressof(entries) if cap else None, cap, C.byref(n), stream), renderer.handle)
    return _components_out(entries[:cap], int(n.value)), int(n.value)


def _grid_args(lo, step, dims):
    lo_c, step_c = _f32(lo).reshape(-1), _f32(step).reshape(-1)
    d = np.asarray(dims)
    if lo_c.size != 3 or step_c.size != 3 or d.size != 3:
        raise NerfError(-1, "lo, step and dims must have three entries each")
    if np.any(d != np.floor(d)) or np.any(np.abs(d) >= 2 ** 31):
        raise NerfError(-1, "dims must be integers")
    dims_c = np.ascontiguousarray(d.reshape(-1), dtype=np.int32)
    n = int(np.prod(dims_c.astype(np.int64))) if np.all(dims_c > 0) else 0     # a dim <= 0: the library refuses the call
    return lo_c, step_c, dims_c, n


def unpack_occupancy(bits, dims):
    """The occupancy words of density_grid -> bool (nz, ny, nx): bit b of word w is linear cell 32 w + b, x fastest."""
    nx, ny, nz = (int(v) for v in dims)
    n = nx * ny * nz
    words = np.ascontiguousarray(bits, dtype="<u4").reshape(-1)
    if nx <= 0 or ny <= 0 or nz <= 0 or words.size != (n + 31) // 32:
        raise NerfError(-1, "bits must hold ceil(nx * ny * nz / 32) words")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool).reshape(nz, ny, nx)


def load_network_from_dir(renderer, which, directory):
    """load_network_from_dir (src/lib.rs:108-174): shapes.txt + <name>.bin, assembled by tensor name."""
    check(renderer._L.nerf_load_network_dir(renderer.handle, which, str(directory).encode()), renderer.handle)
    return Network(renderer, which)


def pack_network_dir(directory, blob_path):
    """Convert a reference-format weight directory into the packed one-memcpy blob (host-only)."""
    check(_lib.load_library().nerf_pack_network_dir(str(directory).encode(), str(blob_path).encode()))


def load_network_blob(renderer, which, blob_path):
    check(renderer._L.nerf_load_network_blob(renderer.handle, which, str(blob_path).encode()), renderer.handle)
    return Network(renderer, which)


class Camera:
    """struct Camera (src/lib.rs:197-211)."""

    def __init__(self, c, samples_per_ray=64):
        self.c = c
        self.samples_per_ray = samples_per_ray

    nx = property(lambda self: self.c.nx)
    ny = property(lambda self: self.c.ny)
    near = property(lambda self: self.c.near)
    far = property(lambda self: self.c.far)
    pos = property(lambda self: np.array(list(self.c.pos), np.float32))
    dir = property(lambda self: np.array(list(self.c.dir), np.float32))
    up = property(lambda self: np.array(list(self.c.up), np.float32))


def camera_from_samples(samples, width, height, coarse_samples_per_ray=64):
    """camera_from_samples (src/lib.rs:614-645).  `samples` is the parsed JSON (dict) or a path to it."""
    L = _lib.load_library()
    c = CCamera()
    if isinstance(samples, (str, bytes)) or hasattr(samples, "__fspath__"):
        import os
        check(L.nerf_camera_from_json(os.fspath(samples).encode() if not isinstance(samples, bytes) else samples,
                                      width, height, C.byref(c)))
    else:
        try:
            o = _f32(samples["camera_origin"]); fw = _f32(samples["camera_forward"]); up = _f32(samples["camera_up"])
            hwf = _f32(samples["hwf"]); near = float(samples["near"]); far = float(samples["far"])
        except (KeyError, TypeError, ValueError) as e:
            raise NerfError(-7, f"camera JSON: missing or malformed key {e}")
        check(L.nerf_camera_from_values(near, far, _p(o), _p(fw), _p(up), _p(hwf), width, height, C.byref(c)))
    return Camera(c, coarse_samples_per_ray)


def camera_from_pose(c2w, hwf, near, far, width, height, coarse_samples_per_ray=64):
    """Camera from a 3x4 camera-to-world matrix (the JSON's "camera_matrix") and hwf = (H, W, focal)."""
    m = _f32(np.asarray(c2w)[:3, :4]).reshape(-1)
    c = CCamera()
    check(_lib.load_library().nerf_camera_from_pose(_p(m), float(hwf[0]), float(hwf[1]), float(hwf[2]), float(near), float(far),
                                                  width, height, C.byref(c)))
    return Camera(c, coarse_samples_per_ray)


class RenderOpts:
    def __init__(self, n_coarse=64, n_fine=128, coarse_only=False, crop=None, ssaa=1, seed=0, dtype="f32", skip_empty=False,
                 skip_dead=False, hybrid_sampling=False, certify_zero=False, band=None):
        self.band = tuple(int(v) for v in band) if band else None   # (index, count, stripe_rows): nerf_render_opts.band_*
        self.hybrid_sampling = bool(hybrid_sampling)
        self.certify_zero = bool(certify_zero)
        self.n_coarse, self.n_fine, self.coarse_only, self.crop, self.ssaa, self.seed = \
            n_coarse, n_fine, coarse_only, crop, ssaa, seed
        self.dtype = _DTYPES[dtype]
        self.skip_empty = bool(skip_empty)
        self.skip_dead = bool(skip_dead)

    def to_c(self):
        o = COpts()
        o.n_coarse, o.n_fine, o.coarse_only = self.n_coarse, self.n_fine, int(self.coarse_only)
        if self.crop:
            o.crop_x0, o.crop_y0, o.crop_w, o.crop_h = self.crop
        o.ssaa, o.seed, o.mlp_dtype, o.skip_empty = self.ssaa, self.seed, self.dtype, int(self.skip_empty)
        o.skip_dead = int(self.skip_dead)
        o.hybrid_sampling = int(self.hybrid_sampling)
        o.certify_zero = int(self.certify_zero)
        if self.band:
            o.band_index, o.band_count, o.band_stripe_rows = self.band
        return o

    def out_shape(self, cam):
        h, w = (self.crop[3], self.crop[2]) if self.crop else (cam.ny, cam.nx)
        if self.band and self.band[1] > 1:
            h = band_rows(h, *self.band)
        return (h, w, 3)


def band_rows(window_rows, index, count, stripe_rows=0):
    """Rows of band `index` of `count` (nerf_band_rows): stripe_rows = 0 contiguous bands, > 0 stripes of that many rows round-robin."""
    n = _lib.load_library().nerf_band_rows(int(window_rows), int(index), int(count), int(stripe_rows))
    if n < 0:
        raise NerfError(n, "band_index / band_count / band_stripe_rows out of range")
    return n


def band_row_indices(window_rows, index, count, stripe_rows=0):
    """The window rows band `index` holds, in the order it holds them (the layout nerf_render_opts.band_* documents)."""
    h, n = int(window_rows), max(int(count), 1)
    if n == 1:
        return np.arange(h)
    if stripe_rows <= 0:
        base, rem = divmod(h, n)
        y0 = index * base + min(index, rem)
        return np.arange(y0, y0 + base + (1 if index < rem else 0))
    rows = np.arange(h)
    return rows[(rows // stripe_rows) % n == index]


def render_image(coarse, fine, camera, fine_samples_per_ray=128, *, seed=0, coarse_only=False, crop=None, ssaa=1,
                 dtype="f32", skip_empty=False, skip_dead=False, hybrid_sampling=False, certify_zero=False, band=None, return_stats=False,
                 device_out=None, stream=0, aux=False, device_depth=None, device_opacity=None):
    """render_image (src/lib.rs:474-565) -> (h, w, 3) float32 linear RGB.

    aux=True: (rgb, depth, opacity), the two maps (h, w) float32 as nerf_render_image_aux defines them (expected distance along the
    unit ray, accumulated weight); followed by the stats if return_stats.  With device_out, device_depth / device_opacity are the maps'
    device pointers (either may be None).

    band = (index, count, stripe_rows): only that band of the window's rows, packed (nerf_render_opts.band_*).

    coarse/fine: Network objects of one Renderer; camera.samples_per_ray is the coarse sample count.
    device_out: optional raw device pointer (int) to receive the image instead of a host array (asynchronous on
    `stream`; returns None / stats)."""
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    opts = RenderOpts(camera.samples_per_ray, fine_samples_per_ray, coarse_only, crop, ssaa, seed, dtype, skip_empty, skip_dead, hybrid_sampling, certify_zero, band)
    o = opts.to_c()
    st = CStats()
    if device_out is not None:
        if aux:
            check(R._L.nerf_render_image_aux_device(R.handle, C.byref(camera.c), C.byref(o), device_out, device_depth, device_opacity, stream,
                                                    C.byref(st) if return_stats else None), R.handle)
        else:
            check(R._L.nerf_render_image_device(R.handle, C.byref(camera.c), C.byref(o), device_out, stream,
                                                C.byref(st) if return_stats else None), R.handle)
        return Stats(st) if return_stats else None
    shape = opts.out_shape(camera)
    if shape[0] <= 0 or shape[1] <= 0:
        raise NerfError(-1, "this band has no rows (more bands than rows)" if opts.band and opts.band[1] > 1 and shape[1] > 0 and
                        (crop[3] if crop else camera.ny) > 0 else "crop window outside the frame")
    out = np.empty(shape, np.float32)
    if aux:
        depth, opacity = np.empty(shape[:2], np.float32), np.empty(shape[:2], np.float32)
        check(R._L.nerf_render_image_aux(R.handle, C.byref(camera.c), C.byref(o), _p(out), _p(depth), _p(opacity), C.byref(st)), R.handle)
        return (out, depth, opacity, Stats(st)) if return_stats else (out, depth, opacity)
    check(R._L.nerf_render_image(R.handle, C.byref(camera.c), C.byref(o), _p(out), C.byref(st)), R.handle)
    return (out, Stats(st)) if return_stats else out


def render_image_rgba8(coarse, fine, camera, fine_samples_per_ray=128, *, background=None, alpha="opaque", seed=0, coarse_only=False,
                       crop=None, ssaa=1, dtype="f32", skip_empty=False, skip_dead=False, hybrid_sampling=False, certify_zero=False,
                       band=None, return_stats=False, device_out=None, stream=0):
    """The display-ready frame (nerf_render_image_rgba8; the reference's render_image_rgba, src/lib.rs:700-726) -> (h, w, 4) uint8,
    R,G,B,A per pixel, packed on the device.

    background: None (white, the reference) or (R, G, B) floats.  alpha: "opaque" (colour over the background, alpha 255),
    "premultiplied" (colour sum_i w_i c_i, alpha = opacity; the background is ignored) or "straight" (colour / opacity).
    The other options are render_image's.  device_out: raw device pointer (int) of h * w * 4 bytes, asynchronous on `stream`
    (returns None / stats)."""
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    opts = RenderOpts(camera.samples_per_ray, fine_samples_per_ray, coarse_only, crop, ssaa, seed, dtype, skip_empty, skip_dead, hybrid_sampling, certify_zero, band)
    o = opts.to_c()
    st = CStats()
    keep, bg = _background(background)
    if device_out is not None:
        check(R._L.nerf_render_image_rgba8_device(R.handle, C.byref(camera.c), C.byref(o), bg, _alpha(alpha), device_out, stream,
                                                  C.byref(st) if return_stats else None), R.handle)
        return Stats(st) if return_stats else None
    shape = opts.out_shape(camera)
    if shape[0] <= 0 or shape[1] <= 0:
        raise NerfError(-1, "crop window outside the frame")
    out = np.empty(shape[:2] + (4,), np.uint8)
    check(R._L.nerf_render_image_rgba8(R.handle, C.byref(camera.c), C.byref(o), bg, _alpha(alpha), out.ctypes.data_as(u8p), C.byref(st)), R.handle)
    return (out, Stats(st)) if return_stats else out


def _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype):
    return RenderOpts(n_coarse, fine_samples_per_ray, coarse_only, None, 1, seed, dtype).to_c()


def _ray_args(origins, dirs, bounds):
    """origins (3,) or (n, 3), dirs (n, 3), bounds None or (n, 2) -> contiguous float32 arrays and n, or NerfError."""
    d = _f32(dirs)
    if d.ndim != 2 or d.shape[1] != 3:
        raise NerfError(-1, "dirs must be an (n, 3) array")
    n = d.shape[0]
    o = _f32(origins)
    if o.shape not in ((3,), (n, 3)):
        raise NerfError(-1, "origins must have shape (3,) or (n, 3)")
    b = None if bounds is None else _f32(bounds)
    if b is not None and b.shape != (n, 2):
        raise NerfError(-1, "bounds must be an (n, 2) array of (near, far)")
    return o, d, b, n


def _ptr(a):
    """A numpy array -> the pointer the C ABI takes; None and raw device pointers (ints) pass."""
    if not isinstance(a, np.ndarray):
        return a
    return a.ctypes.data_as({np.dtype(np.uint32): u32p, np.dtype(np.uint8): u8p}.get(a.dtype, f32p))


def _quantile_args(quantiles):
    """1 .. 8 quantiles in (0, 1] -> a contiguous float32 vector, or NerfError."""
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(quantiles, dtype=np.float32)))
    if qs.ndim != 1 or not 1 <= qs.size <= 8:
        raise NerfError(-1, "quantiles must hold between 1 and 8 values")
    if not np.all(np.isfinite(qs) & (qs > 0) & (qs <= 1)):
        raise NerfError(-1, "a quantile must be finite and lie in (0, 1]")
    return qs


def _ray_head(origins, n_origins, dirs, n_rays, normalize, near, far, bounds, rng_index, opts, bg, rgb, depth, opacity):
    """What every nerf_render_rays* entry point takes from `origins` to `opacity_out`; arrays or raw device pointers."""
    return (_ptr(origins), int(n_origins), _ptr(dirs), int(n_rays), int(bool(normalize)), float(near), float(far), _ptr(bounds), _ptr(rng_index),
            C.byref(opts), bg, _ptr(rgb), _ptr(depth), _ptr(opacity))


def render_rays(coarse, fine, origins, dirs, near, far, fine_samples_per_ray=128, *, n_coarse=64, bounds=None, normalize=True,
                rng_index=None, seed=0, coarse_only=False, dtype="f32", background=None, aux=False, return_stats=False, normals_h=None,
                certify_zero=False, quantiles=None):
    """The caller's rays instead of a camera's (nerf_render_rays) -> rgb (n, 3) float32.

    origins: (3,) -- one origin for every ray -- or (n, 3); dirs: (n, 3), normalised on the device unless normalize=False (the caller
    then promises unit length); near, far: the interval every ray samples, unless bounds (n, 2) = (near, far) per ray is given;
    rng_index: (n,) uint32, the index ray r draws its samples from (None: r) -- a camera's rays with rng_index = row * nx + col give the
    bits of render_image.  n_coarse + fine_samples_per_ray samples, seed, coarse_only, dtype as in render_image; background: None
    (white) or (R, G, B).  aux=True: (rgb, depth (n,), opacity (n,)) as render_image(aux=True); the stats follow if return_stats.
    normals_h: a central-difference step h (finite, > 0) -> the per-ray normals (n, 3) follow the other arrays (the fourth array with
    aux=True): minus the weighted sum of the density gradients at the live samples, normalised; zero for a ray without a live sample
    (nerf_render_rays_normals).  Colour, depth and opacity keep their bits.
    certify_zero=True: zero certification inside every pass, as render_image(certify_zero=True) -- the same bits for a fraction of the
    network evaluations (nerf_render_rays_certified; dtype f32, bf16x3 or f16x2; not with normals_h); the stats carry the audit.
    quantiles: 1 .. 8 values q in (0, 1] -> depth_q (n_q, n) follows the other arrays (nerf_render_rays_quantiles): per ray the position of
    the first sample at which the running sum of the weights reaches q -- 0.5 is the median depth --, 0 for a ray that never reaches it.
    Colour, depth and opacity keep their bits.  Not together with normals_h or certify_zero.
    The other per-pixel options of render_image (crop, ssaa, bands, skip_empty, skip_dead, hybrid_sampling) do not exist for rays."""
    if certify_zero and normals_h is not None:
        raise NerfError(-1, "normals are not offered on a certified batch")
    if quantiles is not None and (certify_zero or normals_h is not None):
        raise NerfError(-1, "quantiles are offered on a plain batch only: not with normals_h or certify_zero")
    qs = None if quantiles is None else _quantile_args(quantiles)
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    o, d, b, n = _ray_args(origins, dirs, bounds)
    idx = None if rng_index is None else np.ascontiguousarray(rng_index, dtype=np.uint32)
    if idx is not None and idx.shape != (n,):
        raise NerfError(-1, "rng_index must have one entry per ray")
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    keep, bg = _background(background)
    rgb = np.empty((n, 3), np.float32)
    depth, opacity = (np.empty(n, np.float32), np.empty(n, np.float32)) if aux else (None, None)
    st = CStats()
    head = _ray_head(o, 1 if o.ndim == 1 else n, d, n, normalize, near, far, b, idx, opts, bg, rgb, depth, opacity)
    if certify_zero:
        check(R._L.nerf_render_rays_certified(R.handle, *head, C.byref(st)), R.handle)
    elif qs is not None:
        depth_q = np.empty((qs.size, n), np.float32)
        check(R._L.nerf_render_rays_quantiles(R.handle, *head, _p(qs), qs.size, _p(depth_q), C.byref(st)), R.handle)
    elif normals_h is None:
        check(R._L.nerf_render_rays(R.handle, *head, C.byref(st)), R.handle)
    else:
        normals = np.empty((n, 3), np.float32)
        check(R._L.nerf_render_rays_normals(R.handle, *head, float(normals_h), _p(normals), C.byref(st)), R.handle)
    out = (rgb, depth, opacity) if aux else (rgb,)
    if normals_h is not None:
        out += (normals,)
    if qs is not None:
        out += (depth_q,)
    if return_stats:
        out += (Stats(st),)
    return out if len(out) > 1 else out[0]


def render_rays_device(coarse, fine, d_origins, n_origins, d_dirs, n_rays, near, far, fine_samples_per_ray, d_rgb, *, n_coarse=64,
                       d_bounds=None, normalize=True, d_rng_index=None, seed=0, coarse_only=False, dtype="f32", background=None,
                       d_depth=None, d_opacity=None, stream=0, return_stats=False, d_normals=None, normals_h=None, certify_zero=False,
                       d_depth_q=None, quantiles=None):
    """nerf_render_rays_device: raw device pointers (ints; d_bounds, d_rng_index, d_depth, d_opacity may be None), asynchronous on
    `stream` (n_origins == 1 reads the origin back first and synchronises the stream once; return_stats synchronises it at the end).
    n_origins is 1 or n_rays.  d_normals (n_rays x 3 floats) together with normals_h: nerf_render_rays_normals_device, which
    synchronises the stream once per pass to read that pass's live count.  certify_zero=True: nerf_render_rays_certified_device, which
    always synchronises the stream before returning (the audit is read on the host); not with normals.  d_depth_q (n_q x n_rays floats)
    together with quantiles (host values): nerf_render_rays_quantiles_device; not with normals or certify_zero.  Returns None / the stats."""
    if (d_normals is None) != (normals_h is None):
        raise NerfError(-1, "d_normals and normals_h go together")
    if (d_depth_q is None) != (quantiles is None):
        raise NerfError(-1, "d_depth_q and quantiles go together")
    if quantiles is not None and (certify_zero or d_normals is not None):
        raise NerfError(-1, "quantiles are offered on a plain batch only: not with normals_h or certify_zero")
    qs = None if quantiles is None else _quantile_args(quantiles)
    if certify_zero and d_normals is not None:
        raise NerfError(-1, "normals are not offered on a certified batch")
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    keep, bg = _background(background)
    st = CStats()
    head = _ray_head(d_origins, n_origins, d_dirs, n_rays, normalize, near, far, d_bounds, d_rng_index, opts, bg, d_rgb, d_depth, d_opacity)
    if certify_zero:
        check(R._L.nerf_render_rays_certified_device(R.handle, *head, stream, C.byref(st) if return_stats else None), R.handle)
    elif qs is not None:
        check(R._L.nerf_render_rays_quantiles_device(R.handle, *head, _p(qs), qs.size, d_depth_q, stream, C.byref(st) if return_stats else None), R.handle)
    elif d_normals is None:
        check(R._L.nerf_render_rays_device(R.handle, *head, stream, C.byref(st) if return_stats else None), R.handle)
    else:
        check(R._L.nerf_render_rays_normals_device(R.handle, *head, float(normals_h), d_normals, stream, C.byref(st) if return_stats else None), R.handle)
    return Stats(st) if return_stats else None


def _occupancy_args(bits, dims):
    d = np.asarray(dims)
    if d.size != 3 or np.any(d != np.floor(d)) or np.any(np.abs(d) >= 2 ** 31):
        raise NerfError(-1, "dims must be three integers")
    dims_c = np.ascontiguousarray(d.reshape(-1), dtype=np.int32)
    n = int(np.prod(dims_c.astype(np.int64))) if np.all(dims_c > 0) else 0     # a dim <= 0: the library refuses the call
    words = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
    if n > 0 and words.size != (n + 31) // 32:
        raise NerfError(-1, "bits must hold ceil(nx * ny * nz / 32) words")
    return words, dims_c, n


def dilate_occupancy(renderer, bits, dims, radius, return_stats=False):
    """Grow the occupancy words of density_grid by `radius` cells (1..4, Chebyshev distance: a cell is set iff a set cell lies within
    `radius` of it along every axis) -> words of the same layout (nerf_occupancy_dilate); return_stats: (words, count, bounds) as
    density_grid reports them."""
    words, dims_c, n = _occupancy_args(bits, dims)
    out = np.zeros(words.size, np.uint32)
    cnt, bounds = C.c_uint64(0), np.zeros(6, np.int32)
    check(renderer._L.nerf_occupancy_dilate(renderer.handle, words.ctypes.data_as(u32p), dims_c.ctypes.data_as(i32p), int(radius),
                                            out.ctypes.data_as(u32p), C.byref(cnt) if return_stats else None,
                                            bounds.ctypes.data_as(i32p) if return_stats else None), renderer.handle)
    return (out, int(cnt.value), tuple(int(v) for v in bounds)) if return_stats else out


def dilate_occupancy_device(renderer, d_bits, dims, radius, d_out, want_stats=False, stream=0):
    """nerf_occupancy_dilate_device: raw device pointers (ints), asynchronous on `stream`; want_stats synchronises it and returns
    (count, bounds), else None."""
    dims_c = np.ascontiguousarray(np.asarray(dims).reshape(-1), dtype=np.int32)
    cnt, bounds = C.c_uint64(0), np.zeros(6, np.int32)
    check(renderer._L.nerf_occupancy_dilate_device(renderer.handle, d_bits, dims_c.ctypes.data_as(i32p), int(radius), d_out,
                                                   C.byref(cnt) if want_stats else None, bounds.ctypes.data_as(i32p) if want_stats else None,
                                                   stream), renderer.handle)
    return (int(cnt.value), tuple(int(v) for v in bounds)) if want_stats else None


def clip_rays(renderer, bits, lo, step, dims, origins, dirs, near, far, bounds=None, normalize=True, return_count=False, debug_cpu=False):
    """Per ray the span of the occupied cells of a density_grid occupancy (bits over the lattice lo, step, dims) inside the ray's
    [near, far] (nerf_clip_rays) -> (bounds (n, 2) float32, hit (n,) bool): a hit ray's bounds are (t_first, t_last), to be handed to
    render_rays(bounds=...); a missed ray keeps its input (near, far).  origins, dirs, near, far, bounds, normalize as in render_rays.
    return_count: the number of hits follows.  debug_cpu=True runs the same function on the host (nerf_debug_clip_rays; renderer may
    be None) and appends the number of out-of-grid reads the range check refused (always 0)."""
    words, dims_c, _ = _occupancy_args(bits, dims)
    lo_c, step_c = _f32(lo).reshape(-1), _f32(step).reshape(-1)
    if lo_c.size != 3 or step_c.size != 3:
        raise NerfError(-1, "lo and step must have three entries each")
    o, d, b, n = _ray_args(origins, dirs, bounds)
    out, hit = np.empty((n, 2), np.float32), np.empty(n, np.uint8)
    cnt, refused = C.c_uint64(0), C.c_uint64(0)
    tail = (words.ctypes.data_as(u32p), _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), _p(o), 1 if o.ndim == 1 else n, _p(d), n,
            int(bool(normalize)), float(near), float(far), None if b is None else _p(b), _p(out), hit.ctypes.data_as(u8p), C.byref(cnt))
    if debug_cpu:
        check(_lib.load_library().nerf_debug_clip_rays(*tail, C.byref(refused)))
    else:
        check(renderer._L.nerf_clip_rays(renderer.handle, *tail), renderer.handle)
    res = (out, hit.astype(bool))
    if return_count:
        res += (int(cnt.value),)
    if debug_cpu:
        res += (int(refused.value),)
    return res


def clip_rays_device(renderer, d_bits, lo, step, dims, d_origins, n_origins, d_dirs, n_rays, near, far, d_bounds_out, d_hit_out, *,
                     d_bounds=None, normalize=True, want_count=False, stream=0):
    """nerf_clip_rays_device: raw device pointers (ints; d_bounds may be None), asynchronous on `stream`; want_count synchronises it
    and returns the number of hits, else None."""
    lo_c, step_c, dims_c, _ = _grid_args(lo, step, dims)
    cnt = C.c_uint64(0)
    check(renderer._L.nerf_clip_rays_device(renderer.handle, d_bits, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), d_origins, int(n_origins),
                                            d_dirs, int(n_rays), int(bool(normalize)), float(near), float(far), d_bounds, d_bounds_out, d_hit_out,
                                            C.byref(cnt) if want_count else None, stream), renderer.handle)
    return int(cnt.value) if want_count else None


def render_rays_clipped(coarse, fine, bits, lo, step, dims, origins, dirs, near, far, fine_samples_per_ray=128, *, n_coarse=64, bounds=None,
                        normalize=True, rng_index=None, seed=0, coarse_only=False, dtype="f32", background=None, aux=False,
                        return_hit=False, return_stats=False, certify_zero=False):
    """render_rays behind clip_rays, on the device (nerf_render_rays_clipped): the rays that cross an occupied cell of the grid are
    rendered over their clipped bounds -- the bits of render_rays for those rays alone with bounds = clip_rays' and rng_index = their
    own index --, the others get the background, depth 0 and opacity 0 without a network evaluation.  Arguments as render_rays plus
    the grid (bits, lo, step, dims as density_grid / dilate_occupancy give them).  return_hit: hit (n,) bool and the number of hits
    follow the arrays; the stats (those of the compacted batch: n_rays = hits) follow if return_stats.  certify_zero=True: the compacted
    batch is rendered with zero certification (nerf_render_rays_clipped_certified) -- the same bits."""
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    words, dims_c, _ = _occupancy_args(bits, dims)
    lo_c, step_c = _f32(lo).reshape(-1), _f32(step).reshape(-1)
    if lo_c.size != 3 or step_c.size != 3:
        raise NerfError(-1, "lo and step must have three entries each")
    o, d, b, n = _ray_args(origins, dirs, bounds)
    idx = None if rng_index is None else np.ascontiguousarray(rng_index, dtype=np.uint32)
    if idx is not None and idx.shape != (n,):
        raise NerfError(-1, "rng_index must have one entry per ray")
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    keep, bg = _background(background)
    rgb = np.empty((n, 3), np.float32)
    depth, opacity = (np.empty(n, np.float32), np.empty(n, np.float32)) if aux else (None, None)
    hit, cnt, st = np.empty(n, np.uint8), C.c_uint64(0), CStats()
    call = R._L.nerf_render_rays_clipped_certified if certify_zero else R._L.nerf_render_rays_clipped
    head = _ray_head(o, 1 if o.ndim == 1 else n, d, n, normalize, near, far, b, idx, opts, bg, rgb, depth, opacity)
    check(call(R.handle, words.ctypes.data_as(u32p), _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), *head, hit.ctypes.data_as(u8p), C.byref(cnt),
               C.byref(st)), R.handle)
    out = (rgb, depth, opacity) if aux else (rgb,)
    if return_hit:
        out += (hit.astype(bool), int(cnt.value))
    if return_stats:
        out += (Stats(st),)
    return out if len(out) > 1 else out[0]


def render_rays_clipped_device(coarse, fine, d_bits, lo, step, dims, d_origins, n_origins, d_dirs, n_rays, near, far, fine_samples_per_ray,
                               d_rgb, *, n_coarse=64, d_bounds=None, normalize=True, d_rng_index=None, seed=0, coarse_only=False, dtype="f32",
                               background=None, d_depth=None, d_opacity=None, d_hit=None, stream=0, return_stats=False, certify_zero=False):
    """nerf_render_rays_clipped_device: raw device pointers (ints; d_bounds, d_rng_index, d_depth, d_opacity, d_hit may be None).
    Synchronises `stream` once after the clip (the hit count sizes the render); what follows is asynchronous unless return_stats.
    certify_zero=True: nerf_render_rays_clipped_certified_device, which also synchronises the stream before returning.
    Returns the number of hits, or (hits, stats)."""
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    lo_c, step_c, dims_c, _ = _grid_args(lo, step, dims)
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    keep, bg = _background(background)
    cnt, st = C.c_uint64(0), CStats()
    call = R._L.nerf_render_rays_clipped_certified_device if certify_zero else R._L.nerf_render_rays_clipped_device
    head = _ray_head(d_origins, n_origins, d_dirs, n_rays, normalize, near, far, d_bounds, d_rng_index, opts, bg, d_rgb, d_depth, d_opacity)
    check(call(R.handle, d_bits, _p(lo_c), _p(step_c), dims_c.ctypes.data_as(i32p), *head, d_hit, C.byref(cnt), stream,
               C.byref(st) if return_stats else None), R.handle)
    return (int(cnt.value), Stats(st)) if return_stats else int(cnt.value)


def render_image_normals(coarse, fine, camera, fine_samples_per_ray=128, *, h, seed=0, coarse_only=False, crop=None, dtype="f32",
                         background=None, return_stats=False):
    """A camera's window with a normal map -> (rgb (h, w, 3), depth (h, w), opacity (h, w), normals (h, w, 3)) float32.

    A convenience over the ray-batch path: the window's unit directions come from stage_ray_dirs, the origin is camera.pos, near / far
    the camera's and rng_index = row * nx + col, then render_rays(aux=True, normals_h=h).  Colour, depth and opacity are therefore the
    bits of render_image(aux=True) for the same window, seed, sample counts and dtype (with the default white background).  crop =
    (x0, y0, w, h) or None for the whole frame; the per-pixel options of render_image that ray batches refuse (ssaa, bands, the skip
    modes) are not offered.  The stats follow if return_stats."""
    R = coarse.renderer
    c = camera.c
    x0, y0, w, hh = crop if crop else (0, 0, c.nx, c.ny)
    if w <= 0 or hh <= 0 or x0 < 0 or y0 < 0 or x0 + w > c.nx or y0 + hh > c.ny:
        raise NerfError(-1, "crop window outside the frame")
    dirs = R.stage_ray_dirs(camera, x0, y0, w, hh, normalize=True).reshape(-1, 3)
    rows, cols = np.meshgrid(np.arange(y0, y0 + hh), np.arange(x0, x0 + w), indexing="ij")
    pix = (rows * c.nx + cols).reshape(-1).astype(np.uint32)
    out = render_rays(coarse, fine, np.float32(list(c.pos)), dirs, c.near, c.far, fine_samples_per_ray, n_coarse=camera.samples_per_ray,
                      normalize=False, rng_index=pix, seed=seed, coarse_only=coarse_only, dtype=dtype, background=background, aux=True,
                      return_stats=return_stats, normals_h=h)
    rgb, depth, opacity, normals = out[:4]
    shaped = (rgb.reshape(hh, w, 3), depth.reshape(hh, w), opacity.reshape(hh, w), normals.reshape(hh, w, 3))
    return shaped + (out[4],) if return_stats else shaped


def _point_args(quantile, min_opacity, normals_h):
    """The three scalars of a point cloud, checked as the library checks them -> (quantile, min_opacity, h)."""
    q = float(_quantile_args([quantile])[0])
    a = float(min_opacity)
    if not (np.isfinite(a) and 0.0 <= a <= 1.0):
        raise NerfError(-1, "min_opacity must be finite and lie in [0, 1]")
    h = 0.0 if normals_h is None else float(normals_h)
    if not (np.isfinite(h) and h >= 0.0) or (normals_h is not None and h == 0.0):
        raise NerfError(-1, "normals_h must be finite and greater than 0 (None: no normals)")
    return q, a, h


def point_cloud(coarse, fine, origins, dirs, near, far, fine_samples_per_ray=128, *, quantile=0.5, min_opacity=0.5, normals_h=None, n_coarse=64,
                bounds=None, normalize=True, rng_index=None, seed=0, coarse_only=False, dtype="f32", capacity=None, return_stats=False):
    """The coloured point cloud of a ray batch (nerf_render_rays_points) -> a dict of arrays trimmed to the n kept rays, in ray order:
    xyz (n, 3) = origin + direction * depth_q, rgb (n, 3) = the ray's colour over black divided by its opacity, ray (n,) uint32 = the
    ray's index in the batch, depth (n,) = depth_q, opacity (n,), and normals (n, 3) when normals_h (a central-difference step > 0) is
    given -- the bits of render_rays(normals_h=...) for those rays.  A ray is kept iff its opacity >= min_opacity and the running sum of
    its weights reaches `quantile` (0.5: the point sits at the median depth).  The ray arguments are render_rays'.  capacity (points;
    default: one per ray, which always suffices): with fewer, NerfError (code -6) names the count.  The stats follow if return_stats."""
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    o, d, b, n = _ray_args(origins, dirs, bounds)
    idx = None if rng_index is None else np.ascontiguousarray(rng_index, dtype=np.uint32)
    if idx is not None and idx.shape != (n,):
        raise NerfError(-1, "rng_index must have one entry per ray")
    q, a, h = _point_args(quantile, min_opacity, normals_h)
    cap = n if capacity is None else int(capacity)
    if cap < 0:
        raise NerfError(-1, "capacity must not be negative")
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    xyz, rgb = np.empty((cap, 3), np.float32), np.empty((cap, 3), np.float32)
    normals = np.empty((cap, 3), np.float32) if h > 0 else None
    ray, depth, opacity = np.empty(cap, np.uint32), np.empty(cap, np.float32), np.empty(cap, np.float32)
    cnt, st = C.c_size_t(0), CStats()
    check(R._L.nerf_render_rays_points(R.handle, _p(o), 1 if o.ndim == 1 else n, _p(d), n, int(bool(normalize)), float(near), float(far),
                                       None if b is None else _p(b), _ptr(idx), C.byref(opts), q, a, h, cap, _p(xyz), _p(rgb),
                                       None if normals is None else _p(normals), ray.ctypes.data_as(u32p), _p(depth), _p(opacity),
                                       C.byref(cnt), C.byref(st)), R.handle)
    m = int(cnt.value)
    out = {"xyz": xyz[:m], "rgb": rgb[:m], "ray": ray[:m], "depth": depth[:m], "opacity": opacity[:m]}
    if normals is not None:
        out["normals"] = normals[:m]
    return (out, Stats(st)) if return_stats else out


def point_cloud_device(coarse, fine, d_origins, n_origins, d_dirs, n_rays, near, far, fine_samples_per_ray, capacity, d_xyz, d_rgb, *,
                       quantile=0.5, min_opacity=0.5, normals_h=None, d_normals=None, d_ray=None, d_depth=None, d_opacity=None, d_n_points=None,
                       n_coarse=64, d_bounds=None, normalize=True, d_rng_index=None, seed=0, coarse_only=False, dtype="f32", stream=0,
                       want_count=False, return_stats=False):
    """nerf_render_rays_points_device: raw device pointers (ints; the optional ones may be None), `capacity` records per output array.
    d_n_points: a device uint32 that receives the full count.  Asynchronous on `stream` as render_rays_device, unless want_count or
    return_stats (which synchronise it) or normals_h (once per pass).  Returns None, the count, the stats or (count, stats)."""
    if (d_normals is None) != (normals_h is None):
        raise NerfError(-1, "d_normals and normals_h go together")
    R = coarse.renderer
    if fine is not None and fine.renderer is not R:
        raise NerfError(-1, "coarse and fine networks must live in the same Renderer")
    q, a, h = _point_args(quantile, min_opacity, normals_h)
    if int(capacity) < 0:
        raise NerfError(-1, "capacity must not be negative")
    opts = _ray_opts(n_coarse, fine_samples_per_ray, seed, coarse_only, dtype)
    cnt, st = C.c_size_t(0), CStats()
    check(R._L.nerf_render_rays_points_device(R.handle, d_origins, int(n_origins), d_dirs, int(n_rays), int(bool(normalize)), float(near), float(far),
                                              d_bounds, d_rng_index, C.byref(opts), q, a, h, int(capacity), d_xyz, d_rgb, d_normals, d_ray, d_depth,
                                              d_opacity, C.byref(cnt) if want_count else None, d_n_points, stream,
                                              C.byref(st) if return_stats else None), R.handle)
    out = ((int(cnt.value),) if want_count else ()) + ((Stats(st),) if return_stats else ())
    return None if not out else out[0] if len(out) == 1 else out


def render_image_points(coarse, fine, camera, fine_samples_per_ray=128, *, quantile=0.5, min_opacity=0.5, normals_h=None, seed=0,
                        coarse_only=False, crop=None, dtype="f32", return_stats=False):
    """The point cloud of a camera's window: point_cloud over the window's ray batch, built as render_image_normals builds it (unit
    directions from stage_ray_dirs, origin camera.pos, the camera's near / far, rng_index = row * nx + col).  `ray` is the pixel's
    index in the window, row-major."""
    R = coarse.renderer
    c = camera.c
    x0, y0, w, hh = crop if crop else (0, 0, c.nx, c.ny)
    if w <= 0 or hh <= 0 or x0 < 0 or y0 < 0 or x0 + w > c.nx or y0 + hh > c.ny:
        raise NerfError(-1, "crop window outside the frame")
    dirs = R.stage_ray_dirs(camera, x0, y0, w, hh, normalize=True).reshape(-1, 3)
    rows, cols = np.meshgrid(np.arange(y0, y0 + hh), np.arange(x0, x0 + w), indexing="ij")
    pix = (rows * c.nx + cols).reshape(-1).astype(np.uint32)
    return point_cloud(coarse, fine, np.float32(list(c.pos)), dirs, c.near, c.far, fine_samples_per_ray, quantile=quantile,
                       min_opacity=min_opacity, normals_h=normals_h, n_coarse=camera.samples_per_ray, normalize=False, rng_index=pix, seed=seed,
                       coarse_only=coarse_only, dtype=dtype, return_stats=return_stats)


def save_point_cloud_ply(path, cloud):
    """A point_cloud dict as a binary little-endian PLY with zero faces (nerf_save_ply): x y z [nx ny nz] red green blue per vertex."""
    save_ply(path, cloud["xyz"], np.zeros((0, 3), np.uint32), normals=cloud.get("normals"), colours=cloud["rgb"])


GATHER_HOST, GATHER_PEER, GATHER_RCCL = 0, 1, 2
_GATHERS = {"host": 0, "peer": 1, "rccl": 2, 0: 0, 1: 1, 2: 2}


def render_image_multi(renderers, camera, fine_samples_per_ray=128, *, gather="host", seed=0, coarse_only=False, crop=None,
                       ssaa=1, dtype="f32", skip_empty=False, skip_dead=False, hybrid_sampling=False, certify_zero=False, return_stats=False,
                       aux=False):
    """render_image fanned out over several Renderers (one per GPU) inside ONE process, through nerf_render_image_multi:
    row bands on per-context host threads + streams, gathered by direct D2H ("host"), GPU-to-GPU peer copies ("peer") or one
    RCCL all-gather ("rccl").  The reference's counterpart is the rayon fan-out + scatter of src/lib.rs:533-557.
    Every Renderer must have both networks loaded.  aux=True: (rgb, depth, opacity) as render_image(aux=True)
    (nerf_render_image_multi_aux), followed by the stats if return_stats."""
    L = _lib.load_library()
    n = len(renderers)
    handles = (C.c_void_p * n)(*[r.handle for r in renderers])
    opts = RenderOpts(camera.samples_per_ray, fine_samples_per_ray, coarse_only, crop, ssaa, seed, dtype, skip_empty, skip_dead, hybrid_sampling, certify_zero)
    o = opts.to_c()
    shape = opts.out_shape(camera)
    if shape[0] <= 0 or shape[1] <= 0:
        raise NerfError(-1, "crop window outside the frame")
    out = np.empty(shape, np.float32)
    st = (CStats * n)()
    if aux:
        depth, opacity = np.empty(shape[:2], np.float32), np.empty(shape[:2], np.float32)
        check(L.nerf_render_image_multi_aux(handles, n, C.byref(camera.c), C.byref(o), _GATHERS[gather], _p(out), _p(depth), _p(opacity),
                                            st if return_stats else None), renderers[0].handle if n else None)
        return (out, depth, opacity, [Stats(s) for s in st]) if return_stats else (out, depth, opacity)
    check(L.nerf_render_image_multi(handles, n, C.byref(camera.c), C.byref(o), _GATHERS[gather], _p(out), st if return_stats else None),
          renderers[0].handle if n else None)
    return (out, [Stats(s) for s in st]) if return_stats else out


def render_image_multi_rgba8(renderers, camera, fine_samples_per_ray=128, *, gather="host", background=None, alpha="opaque", seed=0,
                             coarse_only=False, crop=None, ssaa=1, dtype="f32", skip_empty=False, skip_dead=False, hybrid_sampling=False,
                             certify_zero=False, return_stats=False):
    """render_image_rgba8 fanned out over several Renderers (nerf_render_image_multi_rgba8): every context packs its own band, the
    gathers move one 32-bit word per pixel.  Options as render_image_multi / render_image_rgba8."""
    L = _lib.load_library()
    n = len(renderers)
    handles = (C.c_void_p * n)(*[r.handle for r in renderers])
    opts = RenderOpts(camera.samples_per_ray, fine_samples_per_ray, coarse_only, crop, ssaa, seed, dtype, skip_empty, skip_dead, hybrid_sampling, certify_zero)
    o = opts.to_c()
    shape = opts.out_shape(camera)
    if shape[0] <= 0 or shape[1] <= 0:
        raise NerfError(-1, "crop window outside the frame")
    out = np.empty(shape[:2] + (4,), np.uint8)
    st = (CStats * n)()
    keep, bg = _background(background)
    check(L.nerf_render_image_multi_rgba8(handles, n, C.byref(camera.c), C.byref(o), _GATHERS[gather], bg, _alpha(alpha),
                                          out.ctypes.data_as(u8p), st if return_stats else None), renderers[0].handle if n else None)
    return (out, [Stats(s) for s in st]) if return_stats else out


def quantize_rgb8(pixels):
    a = _f32(pixels)
    out = np.empty(a.shape, np.uint8)
    _lib.load_library().nerf_quantize_rgb8(_p(a), a.size // 3, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def quantize_rgba8(pixels):
    """pixels_to_rgba (src/lib.rs:582-592): (..., 3) f32 -> (..., 4) u8 with alpha 255."""
    a = _f32(pixels)
    out = np.empty(a.shape[:-1] + (4,), np.uint8)
    _lib.load_library().nerf_quantize_rgba8(_p(a), a.size // 3, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def save_ppm(path, width, height, pixels):
    """save_ppm (src/lib.rs:567-580); pixels: (height, width, 3) or (height*width, 3)."""
    a = _f32(pixels)
    if a.size != width * height * 3:
        raise NerfError(-1, "pixels.len() != width * height")  # assert_eq! src/lib.rs:569
    check(_lib.load_library().nerf_save_ppm(str(path).encode(), width, height, _p(a)))


def save_pfm(path, width, height, values):
    """A depth or opacity map as a one-channel PFM (nerf_save_pfm: "Pf", little-endian, rows bottom-up); values: (height, width)."""
    a = _f32(values)
    if a.size != width * height:
        raise NerfError(-1, "values.len() != width * height")
    check(_lib.load_library().nerf_save_pfm(str(path).encode(), width, height, _p(a)))


def save_pam(path, width, height, rgba):
    """An RGBA8 frame as a PAM (nerf_save_pam: "P7", TUPLTYPE RGB_ALPHA, MAXVAL 255); rgba: (height, width, 4) uint8."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.size != width * height * 4:
        raise NerfError(-1, "rgba.len() != width * height * 4")
    check(_lib.load_library().nerf_save_pam(str(path).encode(), width, height, a.ctypes.data_as(u8p)))


def save_ply(path, vertices, triangles, normals=None, colours=None):
    """An indexed triangle mesh as a binary little-endian PLY (nerf_save_ply): vertices (V, 3) f32, triangles (T, 3) uint32, optional normals
    (V, 3) f32 and colours (V, 3) f32 (written as uchar red / green / blue through quantize_rgb8)."""
    v = _f32(vertices).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    n = None if normals is None else _f32(normals).reshape(-1, 3)
    c = None if colours is None else _f32(colours).reshape(-1, 3)
    if (n is not None and n.shape != v.shape) or (c is not None and c.shape != v.shape):
        raise NerfError(-1, "normals and colours must have one row per vertex")
    check(_lib.load_library().nerf_save_ply(str(path).encode(), v.shape[0], _p(v), None if n is None else _p(n), None if c is None else _p(c),
                                            t.shape[0], t.ctypes.data_as(u32p)))


def load_tf_samples(path):
    """load_tf_samples (src/lib.rs:94-99)."""
    with open(path) as f:
        return json.load(f)
