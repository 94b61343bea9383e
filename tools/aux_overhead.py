#!/usr/bin/env python3
"""What the depth and opacity maps cost: renders the C3 frame (800x800, 64 + 128, seed 0) alternately without and with the maps
(nerf_render_image / nerf_render_image_aux).  The two k_composite instances have different names (k_composite<false> = colour
only, k_composite<true> = with the maps), so a kernel trace separates their times:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/aux_overhead.py --frames 5

It also prints the host wall time per frame of each kind and checks that the colour is the same bits either way."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5, help="frames of each kind, alternating")
    ap.add_argument("--size", type=int, default=800)
    a = ap.parse_args()
    scene = os.path.join(ROOT, "lego_rust")
    S = N.api.load_tf_samples(os.path.join(scene, "tf_reference_samples.json"))
    with N.Renderer(0) as r:
        r.load_scene(scene)
        cam = N.camera_from_samples(S, a.size, a.size, 64)
        ref = N.render_image(r.coarse, r.fine, cam, 128, seed=0)          # warm-up (allocations)
        N.render_image(r.coarse, r.fine, cam, 128, seed=0, aux=True)
        wall = {False: [], True: []}
        for _ in range(a.frames):
            for aux in (False, True):
                t0 = time.perf_counter()
                out = N.render_image(r.coarse, r.fine, cam, 128, seed=0, aux=aux)
                wall[aux].append(time.perf_counter() - t0)
                assert np.array_equal(out[0] if aux else out, ref)
        for aux in (False, True):
            print(f"{'with maps ' if aux else 'colour only'}: median host wall {1e3 * np.median(wall[aux]):.2f} ms over {a.frames} frames")


if __name__ == "__main__":
    main()
