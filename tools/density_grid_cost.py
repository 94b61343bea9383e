#!/usr/bin/env python3
"""What a density grid costs: a 256^3 lattice of the fine network through nerf_density_grid_device, timed with device events, beside the
prediction  N x 982 528 FLOP / (rate of the sigma-only RAY kernel in the same session)  -- that rate comes from nerf_stats.ms_coarse_mlp of
a plain 800 x 800 f32 render, whose coarse pass is nerf_mlp_kernel<false, MLP_MODE_RAYS> and nothing else.  The grid kernel runs the same
trunk and does strictly less per-point input work (no t / direction loads, two integer divisions instead), so the ratio should be ~1.

    python tools/density_grid_cost.py [--n 256] [--launches 7] [--out profiles/density_grid_cost.txt]

No threshold is applied to the result: the numbers are written down, DESIGN 4.10 quotes them.  Device memory and events come from the HIP
runtime the library is linked against (through the library's handle): no other GPU stack in the process."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_SIGMA = 982_528


class Hip:
    def __init__(self, L):
        self.L = L
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        L.hipEventSynchronize.argtypes = [C.c_void_p]
        L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), nbytes))
        return p.value

    def event(self):
        e = C.c_void_p()
        self.ok(self.L.hipEventCreate(C.byref(e)))
        return e

    def elapsed_ms(self, fn):
        """Device time of what fn enqueues on the default stream."""
        a, b = self.event(), self.event()
        self.ok(self.L.hipEventRecord(a, None))
        fn()
        self.ok(self.L.hipEventRecord(b, None))
        self.ok(self.L.hipEventSynchronize(b))
        ms = C.c_float()
        self.ok(self.L.hipEventElapsedTime(C.byref(ms), a, b))
        return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="cells per axis")
    ap.add_argument("--launches", type=int, default=7, help="timed launches per form, after one warm-up (>= 5)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert args.launches >= 5
    import numpy as np
    import nerf_rs_amd as N

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = os.path.join(ROOT, "lego_rust")
    with N.Renderer(0) as r:
        r.load_scene(scene)
        info = r.device_info()
        say(f"device {info['arch']} ({info['n_cus']} CUs); {args.launches} timed launches per form after one warm-up; device events")
        # ---- the yardstick: the sigma-only ray kernel of a plain 800 x 800 render (coarse pass, 64 samples per ray)
        cam = N.camera_from_samples(os.path.join(scene, "tf_reference_samples.json"), 800, 800, 64)
        hip = Hip(N.load_library())
        d_img = hip.malloc(800 * 800 * 3 * 4)
        stream = 0                                                 # the default stream, for the events as well
        rates = []
        for i in range(4):
            st = N.render_image(r.coarse, r.fine, cam, 128, seed=0, return_stats=True, device_out=d_img, stream=stream)
            if i:                                                  # the first frame warms up
                rates.append(st.n_coarse_points * FLOP_SIGMA / (st.ms_coarse_mlp * 1e-3))
                say(f"  800x800 render {i}: coarse MLP {st.ms_coarse_mlp:.3f} ms for {st.n_coarse_points} points = {rates[-1] / 1e12:.2f} TFLOP/s")
        rate = statistics.median(rates)
        say(f"sigma-only ray kernel: median {rate / 1e12:.2f} TFLOP/s = {rate / FLOP_SIGMA / 1e6:.2f} M points/s")

        # ---- the grid: the lego frustum's bounding region, n^3 cells of the fine network
        n = args.n
        cells = n ** 3
        lo = (-1.3, -1.3, -0.8)
        step = (2.6 / n, 2.6 / n, 2.2 / n)
        predicted_ms = cells * FLOP_SIGMA / rate * 1e3
        say(f"grid {n}^3 = {cells} cells of the fine network; predicted {predicted_ms:.2f} ms")
        d_sig, d_bits = hip.malloc(cells * 4), hip.malloc((cells + 31) // 32 * 4)

        def timed(label, **kw):
            ms = []
            for i in range(args.launches + 1):
                t = hip.elapsed_ms(lambda: r.fine.density_grid_device(lo, step, (n, n, n), stream=stream, **kw))
                if i:
                    ms.append(t)
            med = statistics.median(ms)
            say(f"  {label:<34s} median {med:8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  = {med / predicted_ms:.4f} x the prediction, "
                f"{cells / med / 1e3:.2f} M points/s")
            return med

        t_sigma = timed("sigma only (4 N bytes out)", d_sigma=d_sig)
        t_both = timed("sigma + occupancy words", d_sigma=d_sig, threshold=10.0, d_bits=d_bits)
        t_bits = timed("occupancy words only (N / 8 bytes)", threshold=10.0, d_bits=d_bits)
        t_stats = timed("occupancy words + count + bounds", threshold=10.0, d_bits=d_bits, want_stats=True)
        count, bounds = r.fine.density_grid_device(lo, step, (n, n, n), threshold=10.0, d_bits=d_bits, want_stats=True, stream=stream)
        say(f"k_occupancy_stats + its 32-byte copy back: {t_stats - t_bits:+.3f} ms on top of the words-only launch ({cells // 8} bytes in)")
        say(f"occupied at sigma > 10: {count} of {cells} cells ({count / cells:.2%}), index bounds {bounds}")
        say(f"ratio grid / prediction: {t_sigma / predicted_ms:.4f} (sigma only), {t_bits / predicted_ms:.4f} (occupancy only); "
            f"sigma + occupancy against sigma only: {t_both / t_sigma:.4f}")
        # host entry point, for scale: staging + 4 N bytes over PCIe
        t0 = time.perf_counter()
        sig, bits, cnt, bnd = r.fine.density_grid(lo, step, (n, n, n), threshold=10.0)
        say(f"host entry point (sigma + words + statistics copied back): {1e3 * (time.perf_counter() - t0):.1f} ms wall; count {cnt}")
        assert cnt == count and tuple(bnd) == tuple(bounds) and int((sig > np.float32(10.0)).sum()) == cnt
        for p in (d_img, d_sig, d_bits):
            hip.L.hipFree(p)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
