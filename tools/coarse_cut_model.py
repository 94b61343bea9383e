#!/usr/bin/env python3
"""CPU model for the coarse cut of the f32 sampling launch (mlp_layout.h RayCutWalk).

The resampler gives every coarse sample behind the reference's T < 1e-4 cut the weight 0 whatever its sigma (src/lib.rs:273-279), so the
sampling launch need not evaluate it -- if the launch can know.  A workgroup that walks the samples of a pixel block front to back knows once
ALL rays of the block are cut.  This model counts, on strips of 32 x 4 pixels of the bench view (four 8 x 4 pixel blocks side by side) with the
oracle's coarse and fine samples and densities (render_ray_debug) and a float32 restatement of compute_weights' transmittance walk:

  * the share of coarse samples behind their own ray's cut (the bound of any mapping);
  * the share in skippable workgroup tiles of the shipped mapping: an 8 x 4 pixel block x 4 sample indices per tile, a tile is skippable when it
    starts behind the last of the block's 32 cuts;
  * the same at one-index granularity for the 8 x 4 block, and for the grouped alternative, a 32 x 4 strip x one index per tile (128 rays must be cut);
  * for the record, the fine pass: the share of fine samples behind their ray's cut, and the share of workgroup tiles of the depth-ordered mapping
    (128 consecutive entries of an 8 x 4 block's depth-sorted samples, tools/depth_order_model.py) all of whose samples are.

Reads only oracle/ and lego_rust/.  Writes profiles/coarsecut_cpu_model.txt."""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zero_step_model as Z  # noqa: E402

oracle_py = Z.oracle_py
STRIP_W, STRIP_H, BLOCK_W = 32, 4, 8
NC, NF = 64, 128
_STATE = {}


def first_behind(sigma, t, far):
    """float32 restatement of compute_weights' walk (src/lib.rs:261-280): the index of the first sample BEHIND the cut (len(t): the ray is never cut)"""
    sigma, t = np.asarray(sigma, np.float32), np.asarray(t, np.float32)
    delta = np.maximum(np.append(t[1:], np.float32(far)) - t, np.float32(0))
    alpha = np.float32(1) - np.exp(-sigma * delta, dtype=np.float32)
    T = np.float32(1)
    for i in range(len(t)):
        T = np.float32(T * (np.float32(1) - alpha[i]))
        if T < np.float32(1e-4):
            return i + 1
    return len(t)


def _init():
    oracle_py.lib()
    samples = oracle_py.load_samples(os.path.join(Z.SCENE, "tf_reference_samples.json"))
    _STATE.update(nets=tuple(oracle_py.Net(os.path.join(Z.SCENE, k)) for k in ("coarse", "fine")), cam=oracle_py.camera_from_samples(samples, 800, 800),
                  opts=oracle_py.make_opts(NC, NF, seed=0), far=float(samples["far"]))


def _ray(ij):
    """-> (first coarse sample behind the coarse cut, t of the merged fine samples, first fine sample behind the fine cut)"""
    d = oracle_py.render_ray_debug(_STATE["nets"][0], _STATE["nets"][1], _STATE["cam"], _STATE["opts"], ij[0], ij[1])
    far = _STATE["far"]
    return (first_behind(d["sigma_coarse"], d["t_coarse"], far), np.asarray(d["t_merged"], np.float32).copy(),
            first_behind(d["sigma_fine"], d["t_merged"], far))


def run(pool, seed, strips):
    rng = np.random.default_rng(seed)
    corners = [(STRIP_W * int(rng.integers(0, 800 // STRIP_W)), STRIP_H * int(rng.integers(0, 800 // STRIP_H))) for _ in range(strips)]
    rays = [(y0 + i, x0 + j) for x0, y0 in corners for i in range(STRIP_H) for j in range(STRIP_W)]
    out = pool.map(_ray, rays, chunksize=32)
    cut_c = np.array([o[0] for o in out]).reshape(strips, STRIP_H, STRIP_W)                      # first coarse index behind the cut
    t_f = np.stack([o[1] for o in out]).reshape(strips, STRIP_H, STRIP_W, NC + NF)
    cut_f = np.array([o[2] for o in out]).reshape(strips, STRIP_H, STRIP_W)
    blocks_c = cut_c.reshape(strips, STRIP_H, STRIP_W // BLOCK_W, BLOCK_W).transpose(0, 2, 1, 3).reshape(-1, 32)    # (block, ray)
    last = blocks_c.max(axis=1)                                                                  # behind it every ray of the block is cut
    per_ray = float((NC - cut_c).sum() / (cut_c.size * NC))
    tile4 = float(((NC - 4 * -(-last // 4)) // 4).sum() / (len(last) * (NC // 4)))               # whole 4-index tiles at or behind `last`
    index1 = float((NC - last).sum() / (len(last) * NC))
    strip1 = float((NC - cut_c.reshape(strips, -1).max(axis=1)).sum() / (strips * NC))
    # fine pass: an 8 x 4 block's 32 x 192 samples by depth (key: bits of t, ray, sample -- the order kernel's), tiles of 128
    tb = t_f.reshape(strips, STRIP_H, STRIP_W // BLOCK_W, BLOCK_W, NC + NF).transpose(0, 2, 1, 3, 4).reshape(-1, 32, NC + NF)
    cb = cut_f.reshape(strips, STRIP_H, STRIP_W // BLOCK_W, BLOCK_W).transpose(0, 2, 1, 3).reshape(-1, 32)
    behind = np.arange(NC + NF)[None, None, :] >= cb[:, :, None]
    fine_tiles = 0
    for b in range(len(tb)):
        ray, smp = np.repeat(np.arange(32), NC + NF), np.tile(np.arange(NC + NF), 32)
        order = np.lexsort((smp, ray, tb[b].reshape(-1).view(np.uint32)))
        fine_tiles += int(behind[b].reshape(-1)[order].reshape(-1, 128).all(axis=1).sum())
    fine_tile = fine_tiles / (len(tb) * 32 * (NC + NF) // 128)
    n_blocks = len(last)
    return [f"coarse cut: CPU model on {strips} strips of {STRIP_W} x {STRIP_H} pixels = {n_blocks} blocks of 8 x 4 = {cut_c.size} rays of the 800x800 view, {NC} + {NF} samples, "
            f"seed {seed} (tools/coarse_cut_model.py)",
            f"strips (x0, y0): {corners}",
            f"  rays the coarse network cuts somewhere in near..far                                   {float((cut_c < NC).mean()):.3f}",
            f"  blocks of 8 x 4 all of whose rays are cut                                             {float((last < NC).mean()):.3f}",
            f"  coarse samples behind their own ray's cut                                             {per_ray:.3f}",
            f"  ... in skippable tiles of the shipped mapping (8 x 4 block x 4 indices)               {tile4:.3f}",
            f"  ... at one-index granularity, 8 x 4 block                                             {index1:.3f}",
            f"  ... at one-index granularity, 32 x 4 strip (grouped alternative, 128 rays per tile)   {strip1:.3f}",
            f"  fine samples behind their own ray's cut (for the record)                              {float(behind.mean()):.3f}",
            f"  ... in workgroup tiles of the depth-ordered mapping all behind their cuts             {fine_tile:.3f}", ""], tile4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="0:56,1:56", help="independent draws as seed:strips, 32 x 4-pixel strips of four 8 x 4 blocks each")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(Z.ROOT, "profiles", "coarsecut_cpu_model.txt"))
    args = ap.parse_args()
    oracle_py.build()
    lines, shares = [], []
    with multiprocessing.Pool(args.jobs, initializer=_init) as pool:
        for draw in args.draws.split(","):
            seed, strips = (int(x) for x in draw.split(":"))
            l, share = run(pool, seed, strips)
            lines += l
            shares.append(share)
    verdict = "below 0.15 in a draw: the idea is dead" if min(shares) < 0.15 else "at least 0.15 in every draw: worth building"
    lines.append(f"skippable share of the shipped mapping per draw: {', '.join(f'{s:.3f}' for s in shares)} -- {verdict}")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
