#!/usr/bin/env python3
"""CPU model for wave tiling of the f32 ray-mode MLP kernels (mlp_layout.h wave tiling).

Which 32 points share a wave decides how often a k-step of a 256-wide layer is dead -- its two hidden units zero after the ReLU on all of
them (zero_step_model.py).  Untiled, a wave holds 32 consecutive samples of one ray; tiled, ss consecutive samples of each ray of a tw x th
block of pixels.  This script prices the candidate shapes on the benchmark's own workload:

  * blocks of 8 x 32 pixels of the 800 x 800 bench view (--draws seed:blocks, by default two independent draws of 5 and 6 blocks; the top-left corner a multiple of (8, 32), so every
    candidate's pixel blocks lie in it whole): 256 rays per block;
  * sample positions from the oracle (render_ray_debug, seed 0): 64 coarse, 64 + 128 fine per ray;
  * the trunk restated in numpy (zero_step_model.trunk), checked against the oracle's sigma;
  * a wave tile = (bundle, j): samples j ss .. j ss + ss - 1 of the tw th rays of one bundle, bundles row-major over the block;
  * workgroup arrangement as the kernel's: grouped, the four waves of a workgroup tile hold the same j of four consecutive bundles
    (zero_step_model.group_rays with bundle for ray); "consecutive" = four consecutive wave tiles of one bundle (NERF_RAY_GROUPING=0);
  * zero_step_model.model_time: a chunk lasts as long as its slowest wave, a skipped k-step costs SKIP_COST_MEASURED (0.28) of an executed one.

Reads only oracle/ and lego_rust/.  Writes profiles/wavetile_cpu_model.txt."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zero_step_model as Z  # noqa: E402

oracle_py = Z.oracle_py
BLOCK_H, BLOCK_W = 8, 32
# (tw, th, ss): pixels across, pixels down, consecutive samples per ray
SHAPES = ((1, 1, 32), (8, 1, 4), (4, 2, 4), (4, 4, 2), (8, 4, 1))
PARENT_MS = {"coarse": 249.2, "fine": 707.3, "rest": 3.0}      # kernel-trace medians of the untiled kernels
UNITS = np.stack([32 * (st >> 4) + Z.ROW_OF[st & 15] for st in range(128)])     # (128 k-steps, 2 units)


def wave_live(nz, shape):
    """nz (BLOCK_H, BLOCK_W, spr, 256) bool: unit non-zero at (pixel row, pixel column, sample) -> live[wave tile, 128 k-steps] in the launch's
    wave-tile order (bundle-major, bundles row-major over the block, then j)."""
    tw, th, ss = shape
    spr = nz.shape[2]
    w = nz.reshape(BLOCK_H // th, th, BLOCK_W // tw, tw, spr // ss, ss, 256).any(axis=(1, 3, 5))      # (by, bx, j, unit)
    w = w.reshape(-1, 256)
    return w[:, UNITS[:, 0]] | w[:, UNITS[:, 1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="0:5,1:6", help="independent draws as seed:blocks, 8 x 32-pixel blocks of 256 rays each (default: 1 280 and 1 536 rays)")
    ap.add_argument("--out", default=os.path.join(Z.ROOT, "profiles", "wavetile_cpu_model.txt"))
    args = ap.parse_args()
    oracle_py.build(); oracle_py.lib()
    lines = []
    for draw in args.draws.split(","):
        seed, blocks = (int(x) for x in draw.split(":"))
        lines += run(argparse.Namespace(seed=seed, blocks=blocks)) + [""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


def run(args):
    nets = {k: oracle_py.Net(os.path.join(Z.SCENE, k)) for k in ("coarse", "fine")}
    W = {k: Z.load(os.path.join(Z.SCENE, k)) for k in nets}
    samples = oracle_py.load_samples(os.path.join(Z.SCENE, "tf_reference_samples.json"))
    cam = oracle_py.camera_from_samples(samples, 800, 800)
    opts = oracle_py.make_opts(64, 128, seed=0)
    origin = np.asarray(samples["camera_origin"], np.float32)
    rng = np.random.default_rng(args.seed)
    consumers = {"coarse": list(range(7)), "fine": list(range(8))}      # ReLU-input layers (zero_step_model.main)
    dense_steps = {"coarse": 64, "fine": 72}
    live = {k: {(s, a): [[] for _ in consumers[k]] for s in SHAPES for a in ("grouped", "consecutive")} for k in nets}
    worst = {"coarse": 0.0, "fine": 0.0}
    corners = []
    for _ in range(args.blocks):
        y0, x0 = BLOCK_H * int(rng.integers(0, 800 // BLOCK_H)), BLOCK_W * int(rng.integers(0, 800 // BLOCK_W))
        corners.append((x0, y0))
        pts, sig = {"coarse": [], "fine": []}, {"coarse": [], "fine": []}
        for i in range(y0, y0 + BLOCK_H):
            for j in range(x0, x0 + BLOCK_W):
                d = oracle_py.render_ray_debug(nets["coarse"], nets["fine"], cam, opts, i, j)
                for k, t, s in (("coarse", d["t_coarse"], d["sigma_coarse"]), ("fine", d["t_merged"], d["sigma_fine"])):
                    pts[k].append((origin[None, :] + d["dir_hat"][None, :] * t[:, None]).astype(np.float32))
                    sig[k].append(s)
        for k in nets:
            P, S = np.concatenate(pts[k]), np.concatenate(sig[k])
            acts, s = Z.trunk(W[k], P)
            worst[k] = max(worst[k], float(np.abs(s - S).max() / (1 + np.abs(S).max())))
            spr = P.shape[0] // (BLOCK_H * BLOCK_W)
            for n, li in enumerate(consumers[k]):
                nz = (acts[li] != 0).reshape(BLOCK_H, BLOCK_W, spr, 256)
                for shape in SHAPES:
                    lv = wave_live(nz, shape)
                    live[k][(shape, "consecutive")][n].append(lv)
                    live[k][(shape, "grouped")][n].append(Z.group_rays(lv, spr // shape[2]))
        print(f"block at {(x0, y0)} done", file=sys.stderr)
    n_rays = args.blocks * BLOCK_H * BLOCK_W
    lines = [f"wave tiling: CPU model on {args.blocks} blocks of {BLOCK_H} x {BLOCK_W} pixels = {n_rays} rays of the 800x800 view, seed {args.seed} (tools/wave_tile_model.py)",
             f"blocks (x0, y0): {corners}",
             f"chunk-coupled timing model of zero_step_model.py at skip cost {Z.SKIP_COST_MEASURED}; wave = tw x th pixels x ss consecutive samples", ""]
    best = {}
    for k in ("coarse", "fine"):
        full = k == "fine"
        lines.append(f"{k}: numpy trunk vs oracle sigma: max |d| / (1 + max |sigma|) = {worst[k]:.1e}")
        lines.append(f"  {'tw x th x ss':14s} {'executed ReLU k-steps':>22s} {'time vs dense, grouped':>24s} {'time vs dense, consecutive':>28s}")
        for shape in SHAPES:
            t = {}
            for a in ("grouped", "consecutive"):
                layers = [np.concatenate(l) for l in live[k][(shape, a)]]
                t[a] = Z.model_time(layers, dense_steps[k], full, Z.SKIP_COST_MEASURED)
            ex = float(np.mean([np.concatenate(l).mean() for l in live[k][(shape, "grouped")]]))
            best[(k, shape)] = t["grouped"]
            tag = " (untiled, shipped before)" if shape == (1, 1, 32) else ""
            lines.append(f"  {'%d x %d x %d' % shape:14s} {ex:22.3f} {t['grouped']:24.4f} {t['consecutive']:28.4f}{tag}")
        lines.append("")
    base = {k: best[(k, (1, 1, 32))] for k in ("coarse", "fine")}
    lines.append(f"per pass against the untiled kernel (kernel medians {PARENT_MS['coarse']} ms coarse, {PARENT_MS['fine']} ms fine, {PARENT_MS['rest']} ms everything else):")
    pick = {}
    for k in ("coarse", "fine"):
        shape = min((s for s in SHAPES), key=lambda s: best[(k, s)])
        pick[k] = shape
        for s in SHAPES[1:]:
            r = best[(k, s)] / base[k]
            lines.append(f"  {k:6s} {'%d x %d x %d' % s:12s} x {r:.4f}: {PARENT_MS[k]:.1f} -> {PARENT_MS[k] * r:.1f} ms{'   <- best' if s == shape else ''}")
    ms0 = PARENT_MS["coarse"] + PARENT_MS["fine"] + PARENT_MS["rest"]
    ms1 = sum(PARENT_MS[k] * best[(k, pick[k])] / base[k] for k in ("coarse", "fine")) + PARENT_MS["rest"]
    lines.append(f"frame with the best shape per pass: {ms0:.1f} -> {ms1:.1f} ms, {100 * (ms0 / ms1 - 1):+.1f} % rays/s")
    return lines


if __name__ == "__main__":
    main()
