#!/usr/bin/env python3
"""What zero certification buys a ray batch: the 800 x 800 lego frame's rays as a batch (64 + 128 samples, f32), the plain call and the
certified call alternated in the same process, in three configurations:

    (a) shared origin                                   nerf_render_rays_device            / nerf_render_rays_certified_device
    (b) the same origin repeated per ray                (per-ray origins: k_batch_points + points mode / ray_origins in the certified kernels)
    (c) clipped at threshold 1, dilate 1, 128^3, shared origin      nerf_render_rays_clipped_device / _clipped_certified_device

and render_image(certify_zero=True) of the same camera in the same session, which (a) is to be read against.

    python tools/bench_ray_certify.py [--size 800] [--repeats 3] [--out profiles/ray_certify_bench.txt]

Per configuration: median, min and max of the synchronous wall time of both calls (each is asked for its stats, so each synchronises), the
certified call's n_exec_* shares, and whether its outputs carry the plain call's bits.  No threshold is applied: the numbers are written
down, DESIGN 4.16 quotes them."""
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
    ap.add_argument("--size", type=int, default=800, help="the frame is size x size rays")
    ap.add_argument("--repeats", type=int, default=3, help="timed alternations per configuration, after one warm-up of each call")
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
            f"{args.repeats} alternations per configuration after one warm-up of each call; wall time of the synchronous call")
        d_o, d_oo, d_dirs = upload(cam.pos), upload(np.tile(np.asarray(cam.pos, np.float32), (n, 1))), upload(dirs)
        d_idx = upload(np.arange(n, dtype=np.uint32))
        d_plain, d_cert = hip.malloc(12 * n), hip.malloc(12 * n)
        g = 128
        dims, lo, step = (g, g, g), (-1.3, -1.3, -0.8), (2.6 / g, 2.6 / g, 2.2 / g)
        words = (g ** 3 + 31) // 32
        d_raw, d_grown = hip.malloc(4 * words), hip.malloc(4 * words)
        r.fine.density_grid_device(lo, step, dims, threshold=1.0, d_bits=d_raw, want_stats=True)
        N.dilate_occupancy_device(r, d_raw, dims, 1, d_grown)

        def rays(origins, n_origins, out, certified):
            return N.render_rays_device(r.coarse, r.fine, origins, n_origins, d_dirs, n, cam.near, cam.far, nf, out, n_coarse=nc, normalize=False,
                                        d_rng_index=d_idx, return_stats=True, certify_zero=certified)

        def clipped(out, certified):
            return N.render_rays_clipped_device(r.coarse, r.fine, d_grown, lo, step, dims, d_o, 1, d_dirs, n, cam.near, cam.far, nf, out, n_coarse=nc,
                                                normalize=False, d_rng_index=d_idx, return_stats=True, certify_zero=certified)[1]

        configs = [("(a) shared origin", lambda out, c: rays(d_o, 1, out, c)),
                   ("(b) the same origin repeated per ray", lambda out, c: rays(d_oo, n, out, c)),
                   ("(c) clipped (threshold 1, dilate 1, 128^3), shared origin", clipped)]

        def timed(f):
            t0 = time.perf_counter()
            st = f()
            return time.perf_counter() - t0, st

        def image():
            return N.render_image(r.coarse, r.fine, cam, nf, certify_zero=True, return_stats=True)

        image()                                                             # warm-up: workspaces, clocks
        t_img = []
        for name, call in configs:
            call(d_plain, False); call(d_cert, True)                        # warm-up of this configuration
            t_p, t_c, faster = [], [], []
            for _ in range(args.repeats):
                tp, _ = timed(lambda: call(d_plain, False))
                tc, st = timed(lambda: call(d_cert, True))
                ti, (_, ist) = timed(image)
                t_p.append(tp); t_c.append(tc); t_img.append(ti); faster.append(tc < tp)
            same = np.array_equal(download(d_plain, (n, 3), np.uint32), download(d_cert, (n, 3), np.uint32))
            mp, mc = statistics.median(t_p), statistics.median(t_c)
            say(name)
            say(f"    plain      median {1e3 * mp:8.2f} ms = {n / mp / 1e6:.3f} M rays/s  (min {1e3 * min(t_p):.2f}, max {1e3 * max(t_p):.2f})")
            say(f"    certified  median {1e3 * mc:8.2f} ms = {n / mc / 1e6:.3f} M rays/s  (min {1e3 * min(t_c):.2f}, max {1e3 * max(t_c):.2f})"
                f"  = {mp / mc:.2f} x the plain rate; faster in {sum(faster)} of {len(faster)} alternations; same bits: {same}")
            say(f"    certified: {st.n_rays} rays, exact evaluations coarse {st.n_exec_coarse_trunk / max(st.n_coarse_points, 1):.3f}, fine "
                f"{st.n_exec_fine_trunk / max(st.n_fine_points, 1):.3f}, colour {st.n_exec_colour / max(st.n_fine_points, 1):.3f} of the nominal samples; device "
                f"{st.ms_total:.2f} ms (coarse MLP {st.ms_coarse_mlp:.2f}, fine MLP {st.ms_fine_mlp:.2f}, other {st.ms_other:.2f}); audited "
                f"{st.n_certify_audited}, violations {st.n_certify_violations}, retries {st.n_certify_retries}")
        mi = statistics.median(t_img)
        say(f"render_image(certify_zero=True), same camera, interleaved with every alternation above (host frame included: 7.7 MB come back)")
        say(f"    median {1e3 * mi:8.2f} ms = {n / mi / 1e6:.3f} M rays/s  (min {1e3 * min(t_img):.2f}, max {1e3 * max(t_img):.2f}); device {ist.ms_total:.2f} ms "
            f"(coarse MLP {ist.ms_coarse_mlp:.2f}, fine MLP {ist.ms_fine_mlp:.2f}, other {ist.ms_other:.2f}); exact evaluations coarse "
            f"{ist.n_exec_coarse_trunk / ist.n_coarse_points:.3f}, fine {ist.n_exec_fine_trunk / ist.n_fine_points:.3f}")
        for p in (d_o, d_oo, d_dirs, d_idx, d_plain, d_cert, d_raw, d_grown):
            L.hipFree(p)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
