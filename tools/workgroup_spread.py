#!/usr/bin/env python3
"""Load balance of the two f32 MLP launches of the benchmark frame (800 x 800, 64 + 128, seed 0): every persistent workgroup stamps the
duration of its tile loop (MlpArgs.clock_out; NERF_DEBUG_CLOCK=1: the fine launch, 2: the sampling launch), and a launch lasts as long as its
slowest workgroup.  Prints min / mean / max of the 256 durations and max / mean per launch, for the context switches given on the command
line as NAME=VALUE (e.g. NERF_TILE_ROTATION=0).  One context per launch kind, one warm-up frame and one measured frame each."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    for kv in sys.argv[1:]:
        k, v = kv.split("=", 1)
        os.environ[k] = v
    import nerf_rs_amd as N
    import oracle_py as O
    scene = os.path.join(ROOT, "lego_rust")
    samples = O.load_samples(os.path.join(scene, "tf_reference_samples.json"))
    cam = N.camera_from_samples(samples, 800, 800, 64)
    for mode, what in (("2", "sampling launch <sigma,rays>"), ("1", "full launch <full,rays>")):
        os.environ["NERF_DEBUG_CLOCK"] = mode
        with N.Renderer(0) as r:
            r.load_scene(scene)
            for _ in range(2):
                N.render_image(r.coarse, r.fine, cam, 128, seed=0)
            ms = r.workgroup_clocks()[:, 1].astype(np.float64) / 1e5      # 100 MHz ticks -> ms
        print(f"workgroup-spread {' '.join(sys.argv[1:]) or 'default':40s} {what:30s} min {ms.min():8.3f} mean {ms.mean():8.3f} max {ms.max():8.3f} ms,"
              f" max / mean {ms.max() / ms.mean():.4f}, slowest workgroup {int(ms.argmax())}")


if __name__ == "__main__":
    main()
