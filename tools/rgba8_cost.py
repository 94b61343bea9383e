#!/usr/bin/env python3
"""What the RGBA8 output costs and saves.

1. Kernel times: renders the C3 frame (800x800, 64 + 128, seed 0) in turn as colour only, with the maps, and as RGBA8 with straight
   alpha, so that a kernel trace holds the two k_composite instances of the float entry points, the two with a background and
   k_pack_rgba8 under their own names:

       rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python tools/rgba8_cost.py --frames 3

   `--summarize OUT/.../run_kernel_trace.csv` prints count and median duration of those kernels from such a trace.
2. Host wall time of a display frame in the fastest exact mode (f16x2 + certify_zero): nerf_render_image_rgba8 against
   nerf_render_image + nerf_quantize_rgba8 -- the read-back and CPU quantisation the device pack removes.  The bytes must be equal."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(path):
    times = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_composite" in name or "k_pack_rgba8" in name or "k_box_downsample" in name:
                times.setdefault(name.split("(")[0], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name in sorted(times):
        t = np.array(times[name])
        print(f"{name}: {len(t)} launches, median {np.median(t):.2f} us, min {t.min():.2f}, max {t.max():.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3, help="frames of each kind, in turn")
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--wall-frames", type=int, default=7, help="frames of each kind for the host wall comparison (0: skip)")
    ap.add_argument("--summarize", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    import nerf_rs_amd as N
    scene = os.path.join(ROOT, "lego_rust")
    S = N.api.load_tf_samples(os.path.join(scene, "tf_reference_samples.json"))
    with N.Renderer(0) as r:
        r.load_scene(scene)
        cam = N.camera_from_samples(S, a.size, a.size, 64)
        ref = N.render_image(r.coarse, r.fine, cam, 128, seed=0)          # warm-up (allocations)
        want = N.quantize_rgba8(ref)
        for _ in range(a.frames):
            assert np.array_equal(N.render_image(r.coarse, r.fine, cam, 128, seed=0), ref)
            assert np.array_equal(N.render_image(r.coarse, r.fine, cam, 128, seed=0, aux=True)[0], ref)
            assert np.array_equal(N.render_image_rgba8(r.coarse, r.fine, cam, 128, seed=0), want)
            N.render_image_rgba8(r.coarse, r.fine, cam, 128, seed=0, alpha="straight", background=(0.25, 0.5, 0.75))
        if a.wall_frames:
            fast = dict(seed=0, dtype="f16x2", certify_zero=True)
            want = N.quantize_rgba8(N.render_image(r.coarse, r.fine, cam, 128, **fast))
            assert np.array_equal(N.render_image_rgba8(r.coarse, r.fine, cam, 128, **fast), want)
            wall = {"float + host quantiser": [], "rgba8 on the device": []}
            for _ in range(a.wall_frames):
                t0 = time.perf_counter()
                N.quantize_rgba8(N.render_image(r.coarse, r.fine, cam, 128, **fast))
                t1 = time.perf_counter()
                N.render_image_rgba8(r.coarse, r.fine, cam, 128, **fast)
                t2 = time.perf_counter()
                wall["float + host quantiser"].append(t1 - t0); wall["rgba8 on the device"].append(t2 - t1)
            for k, v in wall.items():
                print(f"{k}: median host wall {1e3 * np.median(v):.2f} ms, min {1e3 * min(v):.2f} ms over {a.wall_frames} frames (f16x2 + certify_zero)")


if __name__ == "__main__":
    main()
