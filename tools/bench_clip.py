#!/usr/bin/env python3
"""What clipping a ray batch to an occupancy grid buys and costs: the 800 x 800 lego frame's rays as a batch (64 + 128 samples, f32)
through nerf_render_rays_device and through nerf_render_rays_clipped_device, alternated in the same run, behind the fine network's 128^3
occupancy over the README's lego box at threshold 1 and 10, dilated by 0, 1 and 2 cells.

    python tools/bench_clip.py [--n 128] [--size 800] [--repeats 3] [--out profiles/clip_bench.txt]

Per configuration: the hit share n_hit / n; wall time and rays/s of both calls (each synchronises: stats are asked for); the device time
of the clip launch alone (HIP events around nerf_clip_rays_device) and of everything the clipped call adds to its render (events around the
call minus nerf_stats.ms_total of the compacted batch: clip, scan, the hit count's round trip, gather, scatter); and the image cost of the
clip in two numbers -- PSNR of the clipped frame against the unclipped one, and the largest unclipped opacity among the rays the clip
called misses (and where such rays end: inside the grid's box or outside it).  The base is nerf_render_rays_device on the same rays in the same process, never the clipped path against itself.
No threshold is applied: the numbers are written down, DESIGN 4.15 quotes them."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from density_grid_cost import Hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="grid cells per axis")
    ap.add_argument("--size", type=int, default=800, help="the frame is size x size rays")
    ap.add_argument("--repeats", type=int, default=3, help="timed alternations per configuration, after one warm-up")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    import numpy as np
    import nerf_rs_amd as N

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = os.path.join(ROOT, "lego_rust")
    nc, nf = 64, 128
    with N.Renderer(0) as r:
        r.load_scene(scene)
        L = N.load_library()
        hip = Hip(L)
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipDeviceSynchronize.argtypes = []

        def upload(a):
            a = np.ascontiguousarray(a)
            p = hip.malloc(max(a.nbytes, 4))
            hip.ok(L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1))
            return p

        def download(p, shape, dtype):
            out = np.empty(shape, dtype)
            hip.ok(L.hipDeviceSynchronize())
            hip.ok(L.hipMemcpy(out.ctypes.data, p, out.nbytes, 2))
            return out

        info = r.device_info()
        cam = N.camera_from_samples(os.path.join(scene, "tf_reference_samples.json"), args.size, args.size, nc)
        dirs = r.stage_ray_dirs(cam, 0, 0, args.size, args.size, normalize=True).reshape(-1, 3)
        n = len(dirs)
        say(f"device {info['arch']} ({info['n_cus']} CUs); {n} rays ({args.size} x {args.size} lego frame) as a batch, {nc} + {nf} samples, f32; "
            f"{args.repeats} alternations per configuration after one warm-up")
        d_o, d_dirs = upload(cam.pos), upload(dirs)
        d_rgb, d_op, d_depth, d_rgb_c, d_hit = hip.malloc(12 * n), hip.malloc(4 * n), hip.malloc(4 * n), hip.malloc(12 * n), hip.malloc(n)
        d_cb = hip.malloc(8 * n)
        g = args.n
        cells, dims, lo, step = g ** 3, (g, g, g), (-1.3, -1.3, -0.8), (2.6 / g, 2.6 / g, 2.2 / g)
        words = (cells + 31) // 32
        d_raw, d_grown = hip.malloc(4 * words), hip.malloc(4 * words)

        def base():
            t0 = time.perf_counter()
            st = N.render_rays_device(r.coarse, r.fine, d_o, 1, d_dirs, n, cam.near, cam.far, nf, d_rgb, n_coarse=nc, normalize=False, d_opacity=d_op,
                                      d_depth=d_depth, return_stats=True)
            return time.perf_counter() - t0, st

        base()                                                              # warm-up: workspaces, clocks
        ref_rgb, ref_op, ref_depth = download(d_rgb, (n, 3), np.float32), download(d_op, (n,), np.float32), download(d_depth, (n,), np.float32)
        # where an unclipped ray ends: its expected termination point o + d * depth / opacity (rays of opacity > 0.5 only)
        solid = ref_op > 0.5
        surface = cam.pos.astype(np.float64) + dirs.astype(np.float64) * (ref_depth / np.where(solid, ref_op, 1.0))[:, None]
        g_lo = np.float64(lo) - 0.5 * np.float64(step)
        g_hi = np.float64(lo) + np.float64(step) * (g - 0.5)
        in_box = np.all((surface >= g_lo) & (surface < g_hi), axis=1)
        say(f"rays with unclipped opacity > 0.5: {int(solid.sum())}; their expected termination point lies outside the grid's box for "
            f"{int((solid & ~in_box).sum())} of them")
        say(f"unclipped frame: {(ref_op > 0).mean():.2%} of the rays have opacity > 0, {(ref_op > 1e-3).mean():.2%} above 1e-3")
        for threshold in (1.0, 10.0):
            count, _ = r.fine.density_grid_device(lo, step, dims, threshold=threshold, d_bits=d_raw, want_stats=True)
            for dilate in (0, 1, 2):
                if dilate:
                    occupied, _ = N.dilate_occupancy_device(r, d_raw, dims, dilate, d_grown, want_stats=True)
                    t_dilate = hip.elapsed_ms(lambda: N.dilate_occupancy_device(r, d_raw, dims, dilate, d_grown))
                d_bits, occupied = (d_grown, occupied) if dilate else (d_raw, count)
                grid = (d_bits, lo, step, dims)

                def clipped():
                    t0 = time.perf_counter()
                    box = {}
                    ms = hip.elapsed_ms(lambda: box.update(out=N.render_rays_clipped_device(
                        r.coarse, r.fine, *grid, d_o, 1, d_dirs, n, cam.near, cam.far, nf, d_rgb_c, n_coarse=nc, normalize=False, d_hit=d_hit,
                        return_stats=True)))
                    hits, st = box["out"]
                    return time.perf_counter() - t0, ms, hits, st

                clipped()                                                   # warm-up of this configuration
                t_base, t_clip, extra, ms_render = [], [], [], []
                for _ in range(args.repeats):
                    tb, _ = base()
                    tc, ms, hits, st = clipped()
                    t_base.append(tb); t_clip.append(tc); extra.append(ms - st.ms_total); ms_render.append(st.ms_total)
                clip_only = statistics.median(hip.elapsed_ms(lambda: N.clip_rays_device(r, *grid, d_o, 1, d_dirs, n, cam.near, cam.far, d_cb, d_hit,
                                                                                     normalize=False)) for _ in range(5))
                rgb_c, hit = download(d_rgb_c, (n, 3), np.float32), download(d_hit, (n,), np.uint8).astype(bool)
                assert hits == int(hit.sum())
                mse = float(np.mean((np.clip(rgb_c, 0, 1).astype(np.float64) - np.clip(ref_rgb, 0, 1).astype(np.float64)) ** 2))
                psnr = float("inf") if mse == 0 else 10.0 * np.log10(1.0 / mse)
                lost = float(ref_op[~hit].max()) if (~hit).any() else 0.0
                se = ((np.clip(rgb_c, 0, 1).astype(np.float64) - np.clip(ref_rgb, 0, 1).astype(np.float64)) ** 2).sum(axis=1)
                miss_solid = ~hit & solid
                mb, mc = statistics.median(t_base), statistics.median(t_clip)
                say(f"threshold {threshold:g}, dilate {dilate}: {occupied} of {cells} cells occupied ({occupied / cells:.2%})"
                    + (f", dilation {t_dilate:.3f} ms" if dilate else ""))
                say(f"    n_hit / n = {hits} / {n} = {hits / n:.2%}")
                say(f"    nerf_render_rays_device          median {1e3 * mb:8.2f} ms wall = {n / mb / 1e6:.3f} M rays/s  (min {1e3 * min(t_base):.2f}, max {1e3 * max(t_base):.2f})")
                say(f"    nerf_render_rays_clipped_device  median {1e3 * mc:8.2f} ms wall = {n / mc / 1e6:.3f} M rays/s  (min {1e3 * min(t_clip):.2f}, max {1e3 * max(t_clip):.2f})"
                    f"  = {mb / mc:.2f} x the unclipped rate")
                say(f"    device time: render of the {hits} hit rays {statistics.median(ms_render):.2f} ms; clip launch alone {clip_only:.3f} ms; "
                    f"clip + scan + count round trip + gather + scatter {statistics.median(extra):.3f} ms (events around the call minus the render)")
                say(f"    image cost: PSNR of the clipped against the unclipped frame {psnr:.2f} dB; largest unclipped opacity among the {n - hits} rays "
                    f"called misses {lost:.4g}; rays with unclipped opacity > 1e-3 called misses: {int((ref_op[~hit] > 1e-3).sum())}")
                say(f"    of the squared error {se[~hit].sum() / max(se.sum(), 1e-300):.1%} sits on the missed rays (the rest: hit rays sampled over their "
                    f"clipped bounds instead of [near, far]); missed rays with unclipped opacity > 0.5: {int(miss_solid.sum())}, of which "
                    f"{int((miss_solid & in_box).sum())} end inside the grid's box")
        for p in (d_o, d_dirs, d_rgb, d_op, d_depth, d_rgb_c, d_hit, d_cb, d_raw, d_grown):
            L.hipFree(p)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
