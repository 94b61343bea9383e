#!/usr/bin/env python3
"""What quantile depths and a point cloud cost beside the ray batch they ride on.

The 800 x 800 lego frame's 640 000 rays at 64 + 128 samples, f32, one origin for every ray, everything resident on the device:
  plain     nerf_render_rays_device with depth and opacity;
  quantile  nerf_render_rays_quantiles_device with quantiles = [0.5]: the compositing launch also writes its weights (4 B per sample)
            and k_ray_quantiles reads them with the positions (8 B per sample);
  points    nerf_render_rays_points_device with h = 0: the same, over black, plus the compaction of the kept rays.
Device time = nerf_stats.ms_total (HIP events on the render stream, first kernel to last); one warm-up call of each form, then
`--frames` calls of each in turn, medians.  --only plain runs the first form alone and needs nothing this change adds: run from a
checkout of the parent commit (same card, processes interleaved) it gives the figure the other two are compared with.

    python tools/surface_cost.py [--frames 7] [--size 800] [--only plain] [--scene DIR]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--only", default=None)
    ap.add_argument("--scene", default=os.path.join(ROOT, "lego_rust"))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import nerf_rs_amd as N
    S = N.api.load_tf_samples(os.path.join(a.scene, "tf_reference_samples.json"))
    W, nc, nf = a.size, 64, 128
    n = W * W
    hipL = N.load_library()       # the HIP runtime the library itself is linked against, looked up through its handle (as tests/test_gpu_density.py does)
    hipL.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hipL.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hipL.hipFree.argtypes = [C.c_void_p]
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert hipL.hipMalloc(C.byref(p), nbytes) == 0
        held.append(p)
        return p.value

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        p = alloc(arr.nbytes)
        assert hipL.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p

    with N.Renderer(0) as r:
        r.load_scene(a.scene)
        cam = N.camera_from_samples(S, W, W, nc)
        dirs = r.stage_ray_dirs(cam, 0, 0, W, W).reshape(-1, 3)
        d_dirs, d_origin, d_idx = upload(dirs), upload(np.float32(list(cam.c.pos))), upload(np.arange(n, dtype=np.uint32))
        d_rgb, d_depth, d_opacity, d_dq = alloc(12 * n), alloc(4 * n), alloc(4 * n), alloc(4 * n)
        d_xyz, d_ray, d_cnt = alloc(12 * n), alloc(4 * n), alloc(4)
        kw = dict(n_coarse=nc, normalize=False, d_rng_index=d_idx, seed=0, return_stats=True)

        def plain():
            return N.render_rays_device(r.coarse, r.fine, d_origin, 1, d_dirs, n, cam.near, cam.far, nf, d_rgb, d_depth=d_depth, d_opacity=d_opacity, **kw)

        def quantile():
            return N.render_rays_device(r.coarse, r.fine, d_origin, 1, d_dirs, n, cam.near, cam.far, nf, d_rgb, d_depth=d_depth, d_opacity=d_opacity,
                                        d_depth_q=d_dq, quantiles=[0.5], **kw)

        def points():
            return N.point_cloud_device(r.coarse, r.fine, d_origin, 1, d_dirs, n, cam.near, cam.far, nf, n, d_xyz, d_rgb, d_ray=d_ray, d_depth=d_depth,
                                        d_opacity=d_opacity, d_n_points=d_cnt, **kw)

        forms = {"plain": plain, "quantile": quantile, "points": points}
        if a.only:
            forms = {a.only: forms[a.only]}
        for f in forms.values():
            f()                                                         # warm-up: allocations
        ms = {k: [] for k in forms}
        for _ in range(a.frames):
            for k, f in forms.items():
                ms[k].append(f().ms_total)
        base = float(np.median(ms[next(iter(forms))]))
        for k in forms:
            v = np.array(ms[k])
            print(f"{a.tag}{k:9s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  ({np.median(v) - base:+.3f} ms = "
                  f"{100 * (np.median(v) - base) / base:+.3f} % of {next(iter(forms))})  [{a.frames} frames, {n} rays x {nc}+{nf}]")
        if "points" in forms:
            cnt = np.zeros(1, np.uint32)
            assert hipL.hipMemcpy(cnt.ctypes.data, d_cnt, 4, 2) == 0
            print(f"{a.tag}points    {int(cnt[0])} of {n} rays kept at quantile 0.5, opacity >= 0.5")
        for p in held:
            hipL.hipFree(p)


if __name__ == "__main__":
    main()
