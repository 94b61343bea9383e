#!/usr/bin/env python3
"""What a mesh costs: the lego lattice of the README example (lo -1.3,-1.3,-0.8, extent 2.6 x 2.6 x 2.2) at n^3 points of the fine network
through nerf_extract_mesh_device, with and without vertex colours, beside nerf_density_grid_device alone on the same lattice in the same
build and session.  Device events on the default stream, warm calls (one untimed call per form first: the workspace is allocated there).

    python tools/mesh_cost.py [--n 128] [--iso 10] [--launches 7] [--out profiles/mesh_cost.txt]
    python tools/mesh_cost.py --components [--out profiles/components_cost.txt]     # + the component filter

--components adds: the same extraction with keep_largest = 1 (labelling, ranking and the filtered classification in front of the mesh
kernels), nerf_lattice_components_device alone on the resident lattice (labels + a table of 16), the component count, the largest
component's share of the inside points and of the vertices, and the bytes returned.

nerf_extract_mesh_device reads the two counts on the host between the counting and the emitting kernels (one stream synchronisation and an
8-byte copy), so the interval between the events contains that round trip: it is the cost a caller sees, not a sum of kernel times.
No threshold is applied to the result: the numbers are written down, DESIGN 4.11 quotes them."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from density_grid_cost import Hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="lattice points per axis")
    ap.add_argument("--iso", type=float, default=10.0)
    ap.add_argument("--launches", type=int, default=7, help="timed calls per form, after one warm-up (>= 5)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--components", action="store_true", help="also time the component filter and the component query")
    args = ap.parse_args()
    assert args.launches >= 5
    import nerf_rs_amd as N

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    scene = os.path.join(ROOT, "lego_rust")
    with N.Renderer(0) as r:
        r.load_scene(scene)
        info = r.device_info()
        n = args.n
        points = n ** 3
        lo, step, dims = (-1.3, -1.3, -0.8), (2.6 / n, 2.6 / n, 2.2 / n), (n, n, n)
        say(f"device {info['arch']} ({info['n_cus']} CUs); fine network, lattice {n}^3 = {points} points, iso {args.iso:g}; "
            f"{args.launches} timed calls per form after one warm-up; device events")
        hip = Hip(N.load_library())
        nv, nt = r.fine.extract_mesh_device(lo, step, dims, args.iso, None, None, None, 0, None, 0)
        say(f"mesh: {nv} vertices, {nt} triangles; bytes returned {12 * nv + 12 * nt} (positions + indices), {24 * nv + 12 * nt} with normals, "
            f"{36 * nv + 12 * nt} with normals and colours, against 4 N = {4 * points} for the sigma lattice")
        d_sig = hip.malloc(points * 4)
        d_v, d_n, d_c, d_t = hip.malloc(max(12 * nv, 4)), hip.malloc(max(12 * nv, 4)), hip.malloc(max(12 * nv, 4)), hip.malloc(max(12 * nt, 4))

        def timed(label, fn):
            ms = []
            for i in range(args.launches + 1):
                t = hip.elapsed_ms(fn)
                if i:
                    ms.append(t)
            med = statistics.median(ms)
            say(f"  {label:<52s} median {med:8.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})")
            return med

        t_grid = timed("nerf_density_grid_device (sigma only)", lambda: r.fine.density_grid_device(lo, step, dims, d_sigma=d_sig))
        t_count = timed("nerf_extract_mesh_device, size query", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, None, None, None, 0, None, 0))
        t_mesh = timed("nerf_extract_mesh_device, positions + triangles", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, d_v, None, None, nv, d_t, nt))
        t_norm = timed("nerf_extract_mesh_device, + normals", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, d_v, d_n, None, nv, d_t, nt))
        t_col = timed("nerf_extract_mesh_device, + normals + colours", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, d_v, d_n, d_c, nv, d_t, nt))
        say(f"on top of the sigma launch: counting {t_count - t_grid:+.3f} ms, emitting positions + triangles {t_mesh - t_count:+.3f} ms, normals "
            f"{t_norm - t_mesh:+.3f} ms, colours ({nv} full evaluations of the network) {t_col - t_norm:+.3f} ms")
        say(f"ratio to the sigma launch alone: {t_mesh / t_grid:.4f} (positions + triangles), {t_norm / t_grid:.4f} (+ normals), {t_col / t_grid:.4f} (+ colours)")
        if args.components:
            fv, ft, n_comp, n_kept = r.fine.extract_mesh_device(lo, step, dims, args.iso, None, None, None, 0, None, 0, keep_largest=1, return_counts=True)
            d_lab = hip.malloc(points * 4)
            comps, n_comp2 = N.lattice_components_device(r, d_sig, dims, args.iso, d_labels=d_lab, table=16)      # d_sig: the timed grid launch's output
            assert n_comp2 == n_comp and n_kept == min(1, n_comp)
            inside = r.fine.density_grid_device(lo, step, dims, d_sigma=None, threshold=args.iso, d_bits=d_lab, want_stats=True)[0]
            say(f"components of sigma > {args.iso:g}: {n_comp} components over {inside} inside points; sizes of the largest "
                f"{[c.n_points for c in comps[:8]]}; the largest holds {100.0 * comps[0].n_points / max(inside, 1):.2f} % of the inside points, "
                f"bounds {comps[0].bounds}")
            say(f"filtered mesh (keep_largest = 1): {fv} vertices ({100.0 * fv / max(nv, 1):.2f} % of {nv}), {ft} triangles ({100.0 * ft / max(nt, 1):.2f} % "
                f"of {nt}); bytes returned {12 * fv + 12 * ft} (positions + indices) against {12 * nv + 12 * nt} unfiltered; a component query "
                f"returns 8 + 32 x table bytes (+ 4 N = {4 * points} only if the labels are asked for)")
            t_filt = timed("nerf_extract_mesh_filtered_device, keep_largest = 1", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, d_v, None, None, nv, d_t, nt,
                                                                                                                   keep_largest=1))
            t_again = timed("nerf_extract_mesh_device, positions + triangles (again)", lambda: r.fine.extract_mesh_device(lo, step, dims, args.iso, d_v, None, None, nv, d_t, nt))
            t_cc = timed("nerf_lattice_components_device, table of 16, no labels", lambda: N.lattice_components_device(r, d_sig, dims, args.iso, table=16))
            t_cc0 = timed("nerf_lattice_components_device, count only", lambda: N.lattice_components_device(r, d_sig, dims, args.iso, table=0))
            t_cc64 = timed("nerf_lattice_components_device, table of 64, no labels", lambda: N.lattice_components_device(r, d_sig, dims, args.iso, table=64))
            t_ccl = timed("nerf_lattice_components_device, table of 16 + labels", lambda: N.lattice_components_device(r, d_sig, dims, args.iso, d_labels=d_lab, table=16))
            say(f"the filter on top of the unfiltered extraction: {t_filt - 0.5 * (t_mesh + t_again):+.3f} ms ({100.0 * (t_filt - 0.5 * (t_mesh + t_again)) / t_grid:.2f} % of the "
                f"sigma launch); the component query alone: {t_cc:.3f} ms ({100.0 * t_cc / t_grid:.2f} % of the sigma launch), of which the 16 ranking passes, the table "
                f"and its bounds {t_cc - t_cc0:+.3f} ms (64 passes: {t_cc64 - t_cc0:+.3f} ms); copying the labels {t_ccl - t_cc:+.3f} ms")
            hip.L.hipFree(d_lab)
        for p in (d_sig, d_v, d_n, d_c, d_t):
            hip.L.hipFree(p)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
