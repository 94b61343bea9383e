#!/usr/bin/env python3
"""What the per-ray normals cost beside the ray batch they ride on.

The 800 x 800 lego frame's 640 000 rays at 64 + 128 samples, f32, through nerf_render_rays_device (the camera's origin for every ray),
without and with normals (h = 1e-3), everything resident on the device.  Device time = nerf_stats.ms_total (HIP events on the render
stream, first kernel to last -- with normals this spans the per-pass read-back of the live count as well); one warm-up call of each form,
then `--frames` calls of each in turn, medians.  Colour, depth and opacity of the two forms must be the same bits.
NERF_DEBUG_NORMALS=1 (set here) makes every normals call print its live share and the split of its own launches -- the sigma-only MLP
launch over the stencil points, and the count / scan / stencil / reduce kernels -- to stderr; this tool repeats the last such line.

    python tools/normals_cost.py [--frames 7] [--size 800] [--step 1e-3]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_batch_cost import Hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--step", type=float, default=1e-3)
    a = ap.parse_args()
    os.environ["NERF_DEBUG_NORMALS"] = "1"                              # read by nerf_create
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
        d_dirs, d_origin = hip.upload(dirs), hip.upload(cam.pos)
        d_idx = hip.upload(np.arange(n, dtype=np.uint32))
        out = {k: (hip.alloc(12 * n), hip.alloc(4 * n), hip.alloc(4 * n)) for k in ("plain", "normals")}
        d_normals = hip.alloc(12 * n)

        def rays(which):
            extra = dict(d_normals=d_normals, normals_h=a.step) if which == "normals" else {}
            return N.render_rays_device(r.coarse, r.fine, d_origin, 1, d_dirs, n, cam.near, cam.far, nf, out[which][0], n_coarse=nc, normalize=False,
                                        d_rng_index=d_idx, seed=0, d_depth=out[which][1], d_opacity=out[which][2], return_stats=True, **extra)

        forms = {"plain": lambda: rays("plain"), "normals": lambda: rays("normals")}
        for f in forms.values():
            f()                                                         # warm-up: allocations
        shapes = ((n, 3), (n,), (n,))
        for got, want, name in zip([hip.download(p, s) for p, s in zip(out["normals"], shapes)], [hip.download(p, s) for p, s in zip(out["plain"], shapes)],
                                   ("rgb", "depth", "opacity")):
            same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
            print(f"with normals: {name} {'bit-identical to' if same else 'DIFFERS from'} the call without ({n} rays)")
            assert same
        normals = hip.download(d_normals, (n, 3))
        opacity = hip.download(out["plain"][2], (n,))
        hit = opacity > 0.5
        facing = (normals * dirs).sum(axis=1) < 0
        print(f"{int((np.abs(normals).sum(axis=1) > 0).sum())} rays carry a normal; of the {int(hit.sum())} rays with opacity > 0.5, {facing[hit].mean():.3f} face the camera")
        ms = {k: [] for k in forms}
        other = {k: [] for k in forms}
        for _ in range(a.frames):
            for k, f in forms.items():
                st = f()
                ms[k].append(st.ms_total); other[k].append(st.ms_other)
        base = float(np.median(ms["plain"]))
        for k in forms:
            v = np.array(ms[k])
            print(f"{k:8s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  ({np.median(v) - base:+.3f} ms = "
                  f"{100 * (np.median(v) - base) / base:+.3f} % of the call without normals); kernels beside the two network passes: median "
                  f"{np.median(other[k]):.3f} ms  [{a.frames} frames, {st.n_passes} pass(es), {n} rays x {nc}+{nf}, h = {a.step:g}]")
        hip.free()


if __name__ == "__main__":
    main()
