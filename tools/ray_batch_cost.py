#!/usr/bin/env python3
"""What a ray batch costs beside the image render it restates.

The 800 x 800 lego frame's 640 000 rays at 64 + 128 samples, f32, three ways, everything resident on the device:
  image    nerf_render_image_aux_device;
  shared   the same rays through nerf_render_rays_device with the camera's origin for every ray (n_origins = 1): k_batch_prepare in
           place of k_ray_dirs + k_stratified, then the image path's launches;
  per-ray  the same rays with the origin repeated per ray (n_origins = n_rays): k_batch_points expands every pass's samples into
           points and per-sample directions (24 B written and read again per sample) for points-mode launches.
Device time = nerf_stats.ms_total (HIP events on the render stream, first kernel to last); one warm-up call of each form, then
`--frames` calls of each in turn, medians.  The three outputs (colour, depth, opacity) must be the same bits.

    python tools/ray_batch_cost.py [--frames 7] [--size 800]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Hip:
    """hipMalloc / hipMemcpy of the runtime the library itself is linked against (loaded by its soname: the same instance)."""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so.7")
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), nbytes) == 0
        self.held.append(p)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert self.L.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.held:
            self.L.hipFree(p)
        self.held = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()
    import nerf_rs_amd as N
    scene = os.path.join(ROOT, "lego_rust")
    S = N.api.load_tf_samples(os.path.join(scene, "tf_reference_samples.json"))
    W, nc, nf = a.size, 64, 128
    n = W * W
    with N.Renderer(0) as r:
        r.load_scene(scene)
        hip = Hip()
        cam = N.camera_from_samples(S, W, W, nc)
        dirs = r.stage_ray_dirs(cam, 0, 0, W, W).reshape(-1, 3)
        d_dirs, d_origin, d_origins = hip.upload(dirs), hip.upload(cam.pos), hip.upload(np.tile(cam.pos, (n, 1)))
        d_idx = hip.upload(np.arange(n, dtype=np.uint32))
        out = {k: (hip.alloc(12 * n), hip.alloc(4 * n), hip.alloc(4 * n)) for k in ("image", "shared", "per-ray")}

        def image():
            return N.render_image(r.coarse, r.fine, cam, nf, seed=0, aux=True, device_out=out["image"][0], device_depth=out["image"][1],
                                  device_opacity=out["image"][2], return_stats=True)

        def rays(which):
            o, k = (d_origin, 1) if which == "shared" else (d_origins, n)
            return N.render_rays_device(r.coarse, r.fine, o, k, d_dirs, n, cam.near, cam.far, nf, out[which][0], n_coarse=nc, normalize=False,
                                        d_rng_index=d_idx, seed=0, d_depth=out[which][1], d_opacity=out[which][2], return_stats=True)

        forms = {"image": image, "shared": lambda: rays("shared"), "per-ray": lambda: rays("per-ray")}
        for f in forms.values():
            f()                                                         # warm-up: allocations
        ref = [hip.download(p, s) for p, s in zip(out["image"], ((n, 3), (n,), (n,)))]
        for which in ("shared", "per-ray"):
            for got, want, name in zip([hip.download(p, s) for p, s in zip(out[which], ((n, 3), (n,), (n,)))], ref, ("rgb", "depth", "opacity")):
                same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
                print(f"{which}: {name} {'bit-identical to' if same else 'DIFFERS from'} the image render's ({n} rays)")
                assert same
        ms = {k: [] for k in forms}
        other = {k: [] for k in forms}
        for _ in range(a.frames):
            for k, f in forms.items():
                st = f()
                ms[k].append(st.ms_total); other[k].append(st.ms_other)
        base = float(np.median(ms["image"]))
        for k in forms:
            v = np.array(ms[k])
            print(f"{k:8s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  ({np.median(v) - base:+.3f} ms = "
                  f"{100 * (np.median(v) - base) / base:+.3f} % of the image render); kernels beside the networks: median {np.median(other[k]):.3f} ms"
                  f"  [{a.frames} frames, {st.n_passes} pass(es), {n} rays x {nc}+{nf}]")
        hip.free()


if __name__ == "__main__":
    main()
