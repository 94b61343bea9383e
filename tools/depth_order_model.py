#!/usr/bin/env python3
"""CPU model for depth-ordered fine waves of the f32 ray-mode MLP kernel (mlp_layout.h DepthOrder).

wave_tile_model.py cuts a wave from a few consecutive sample INDICES of each ray of a pixel block.  In the fine pass every ray places its
importance samples differently, so one index is another depth on every ray.  Here the 64 + 128 fine samples of all rays of a pixel block are
merged by depth t -- key (bits of t, ray-in-block, sample), as the order kernel's -- and the sorted list is cut into waves of 32.  Priced on
the same workload with the same tools as wave_tile_model.py (blocks of 8 x 32 pixels of the bench view, oracle sample positions, the numpy
trunk, the chunk-coupled timing model at skip cost 0.28):

  * the shipped 4 x 2 x 4 static tiling, grouped, as the base line;
  * depth-sorted blocks of 4 x 2, 8 x 2, 8 x 4, 16 x 4 and 32 x 8 pixels, a workgroup tile = four consecutive depth slabs of one block;
  * 8 x 4 with a workgroup tile = the same slab of four neighbouring blocks;
  * load balance: a persistent workgroup c of 256 takes tiles c + 256 k, and a launch's tiles come in periods (64 sample indices in the coarse
    pass, 48 tiles per 8 x 4 block in the fine pass), so c only ever sees some positions j of the period.  The spread of the mean model cost
    per position j says how much slower the slowest class of workgroups is than a balanced launch -- what rotating the assignment removes.

Reads only oracle/ and lego_rust/.  Writes profiles/depthorder_cpu_model.txt."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_tile_model as T  # noqa: E402
import zero_step_model as Z  # noqa: E402

oracle_py = Z.oracle_py
BLOCK_H, BLOCK_W = T.BLOCK_H, T.BLOCK_W
UNITS = T.UNITS
SHIPPED = (4, 2, 4)
# (bw, bh, arrangement): pixels across and down of a depth-sorted block; "slabs" = four consecutive slabs per workgroup tile, "blocks" = one slab of four blocks
SORTED = ((4, 2, "slabs"), (8, 2, "slabs"), (8, 4, "slabs"), (8, 4, "blocks"), (16, 4, "slabs"), (32, 8, "slabs"))
FINE_MS = 695.0   # kernel-trace median of the shipped fine kernel (wave-tiling table)


def sorted_live(nz, t, bw, bh, arrangement):
    """nz (BLOCK_H, BLOCK_W, spr, 256) bool, t (BLOCK_H, BLOCK_W, spr) float32 -> live[wave tile, 128 k-steps] in launch order"""
    spr = nz.shape[2]
    out = []
    for by in range(BLOCK_H // bh):
        for bx in range(BLOCK_W // bw):
            tb = np.ascontiguousarray(t[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw]).reshape(-1).view(np.uint32)
            nb = nz[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw].reshape(-1, 256)
            ray = np.repeat(np.arange(bw * bh), spr)
            smp = np.tile(np.arange(spr), bw * bh)
            order = np.lexsort((smp, ray, tb))
            w = nb[order].reshape(-1, 32, 256).any(axis=1)                     # (slab, unit)
            out.append(w[:, UNITS[:, 0]] | w[:, UNITS[:, 1]])
    if arrangement == "blocks":                                                # wave w of tile (b / 4, slab) = slab of block 4 (b / 4) + w
        a = np.stack(out)                                                      # (block, slab, 128)
        a = a.reshape(-1, 4, a.shape[1], 128).transpose(0, 2, 1, 3)
        return a.reshape(-1, 128)
    return np.concatenate(out)


def tile_costs(layers, dense_steps, full, skip_cost):
    """model_time's numerator per workgroup tile (4 waves), in macro-steps"""
    total = np.zeros(layers[0].shape[0] // 4)
    for li, live in enumerate(layers):
        cost = np.where(live, 1.0, skip_cost)
        if full and li == len(layers) - 1:
            cost = 0.5 * cost.reshape(cost.shape[0], 64, 2).sum(axis=2)
            per_chunk = cost.reshape(cost.shape[0], 8, 8).sum(axis=2)
        else:
            per_chunk = cost.reshape(cost.shape[0], 16, 8).sum(axis=2)
        total += per_chunk.reshape(-1, 4, per_chunk.shape[1]).max(axis=1).sum(axis=1)
    return total + dense_steps


def class_spread(costs, period, classes):
    """tiles come in periods of `period`; a workgroup sees positions j = c mod period for c in one of `classes` residue classes (256 workgroups,
    stride 256): mean cost of the slowest class over the mean of all"""
    per_j = costs.reshape(-1, period).mean(axis=0)
    g = np.gcd(256, period)                                                    # workgroup c sees j = c mod g (mod period: c + 256 k)
    per_class = np.array([per_j[r::g].mean() for r in range(g)])
    assert len(per_class) == classes
    return per_j.min() / per_j.mean(), per_j.max() / per_j.mean(), per_class.max() / per_class.mean()


def run(args):
    nets = {k: oracle_py.Net(os.path.join(Z.SCENE, k)) for k in ("coarse", "fine")}
    Wt = {k: Z.load(os.path.join(Z.SCENE, k)) for k in nets}
    samples = oracle_py.load_samples(os.path.join(Z.SCENE, "tf_reference_samples.json"))
    cam = oracle_py.camera_from_samples(samples, 800, 800)
    opts = oracle_py.make_opts(64, 128, seed=0)
    origin = np.asarray(samples["camera_origin"], np.float32)
    rng = np.random.default_rng(args.seed)
    names = [SHIPPED] + list(SORTED)
    live = {n: [[] for _ in range(8)] for n in names}
    coarse_live = [[] for _ in range(7)]
    corners, worst = [], 0.0
    for _ in range(args.blocks):
        y0, x0 = BLOCK_H * int(rng.integers(0, 800 // BLOCK_H)), BLOCK_W * int(rng.integers(0, 800 // BLOCK_W))
        corners.append((x0, y0))
        pts, sig, ts = {"coarse": [], "fine": []}, {"coarse": [], "fine": []}, []
        for i in range(y0, y0 + BLOCK_H):
            for j in range(x0, x0 + BLOCK_W):
                d = oracle_py.render_ray_debug(nets["coarse"], nets["fine"], cam, opts, i, j)
                for k, t, s in (("coarse", d["t_coarse"], d["sigma_coarse"]), ("fine", d["t_merged"], d["sigma_fine"])):
                    pts[k].append((origin[None, :] + d["dir_hat"][None, :] * t[:, None]).astype(np.float32))
                    sig[k].append(s)
                ts.append(np.asarray(d["t_merged"], np.float32))
        t = np.stack(ts).reshape(BLOCK_H, BLOCK_W, -1)
        for k in nets:
            P, S = np.concatenate(pts[k]), np.concatenate(sig[k])
            acts, s = Z.trunk(Wt[k], P)
            worst = max(worst, float(np.abs(s - S).max() / (1 + np.abs(S).max())))
            spr = P.shape[0] // (BLOCK_H * BLOCK_W)
            for n in range(8 if k == "fine" else 7):
                nz = (acts[n] != 0).reshape(BLOCK_H, BLOCK_W, spr, 256)
                if k == "coarse":
                    coarse_live[n].append(Z.group_rays(T.wave_live(nz, (8, 4, 1)), spr))
                    continue
                live[SHIPPED][n].append(Z.group_rays(T.wave_live(nz, SHIPPED), spr // SHIPPED[2]))
                for name in SORTED:
                    live[name][n].append(sorted_live(nz, t, *name))
        print(f"block at {(x0, y0)} done", file=sys.stderr)
    n_rays = args.blocks * BLOCK_H * BLOCK_W
    lines = [f"depth ordering: CPU model on {args.blocks} blocks of {BLOCK_H} x {BLOCK_W} pixels = {n_rays} rays of the 800x800 view, seed {args.seed} (tools/depth_order_model.py)",
             f"blocks (x0, y0): {corners}",
             f"chunk-coupled timing model of zero_step_model.py at skip cost {Z.SKIP_COST_MEASURED}; numpy trunk vs oracle sigma: max |d| / (1 + max |sigma|) = {worst:.1e}", "",
             f"fine pass ({'wave composition':58s} {'executed ReLU k-steps':>22s} {'model time vs dense':>20s} {'vs shipped':>11s} {'fine kernel':>12s})"]
    base = None
    for name in names:
        layers = [np.concatenate(l) for l in live[name]]
        tm = Z.model_time(layers, 72, True, Z.SKIP_COST_MEASURED)
        ex = float(np.mean([l.mean() for l in layers]))
        base = tm if base is None else base
        what = "shipped 4 x 2 x 4, grouped" if name == SHIPPED else (
            f"depth-sorted {name[0]} x {name[1]}, " + ("4 consecutive slabs per workgroup" if name[2] == "slabs" else "same slab of 4 neighbouring blocks"))
        lines.append(f"  {what:68s} {ex:22.3f} {tm:20.4f} {tm / base:11.4f} {FINE_MS * tm / base:9.1f} ms")
    lines += ["", "load balance: mean model cost per position j of a launch's tile period, relative to the mean over all tiles",
              "(workgroup c of 256 takes tiles c + 256 k: it sees only the positions j = c mod gcd(256, period))"]
    cc = tile_costs([np.concatenate(l) for l in coarse_live], 64, False, Z.SKIP_COST_MEASURED)
    lo, hi, cls = class_spread(cc, 64, 64)
    lines.append(f"  coarse, 8 x 4 x 1 grouped, period 64 (sample index):        per j {lo:.3f} .. {hi:.3f}; slowest of 64 classes {cls:.3f} of balanced")
    for name, what in ((SHIPPED, "fine, shipped 4 x 2 x 4 grouped, period 48 (sample index / 4)"), ((8, 4, "slabs"), "fine, depth-sorted 8 x 4, period 48 (depth rank)")):
        fc = tile_costs([np.concatenate(l) for l in live[name]], 72, True, Z.SKIP_COST_MEASURED)
        lo, hi, cls = class_spread(fc, 48, 16)
        lines.append(f"  {what:62s}: per j {lo:.3f} .. {hi:.3f}; slowest of 16 classes {cls:.3f} of balanced")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="0:6,1:6", help="independent draws as seed:blocks, 8 x 32-pixel blocks of 256 rays each")
    ap.add_argument("--out", default=os.path.join(Z.ROOT, "profiles", "depthorder_cpu_model.txt"))
    args = ap.parse_args()
    oracle_py.build(); oracle_py.lib()
    lines = []
    for draw in args.draws.split(","):
        seed, blocks = (int(x) for x in draw.split(":"))
        lines += run(argparse.Namespace(seed=seed, blocks=blocks)) + [""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
