#!/usr/bin/env python3
"""CPU model for the fine cut of the depth-ordered full f32 launch (mlp_layout.h fine_cut_walk_of).

k_composite gives every fine sample behind the reference's T < 1e-4 cut the weight 0 whatever its sigma and colour (src/lib.rs:273-279).  A
workgroup that walks the ordered tiles of an 8 x 4 pixel block front to back (128 consecutive entries of the block's depth-sorted samples per
tile, 48 tiles at 64 + 128) knows once ALL 32 rays of the block are cut, and leaves the block behind the tile in which the last of them is.
This model counts, on strips of 32 x 4 pixels of the bench view with the oracle's fine samples and densities (render_ray_debug), a float32
restatement of compute_weights' transmittance walk and the order kernel's key (bits of t, ray in block, sample):

  * the share of fine samples behind their own ray's cut (the bound of any mapping);
  * the share of workgroup tiles the walk never starts -- those behind the tile in which the block's last ray is cut;
  * its split into tiles whose 128 densities are all 0 (the empty-tile vote already skips their colour head) and tiles that hold density;
  * for comparison, the share of tiles with density among all tiles, and the share of all sigma > 0 samples that lie in skipped tiles.

Shares code with tools/coarse_cut_model.py (the oracle set-up and the walk), whose own output is unchanged.  Reads only oracle/ and lego_rust/.
Writes profiles/finecut_cpu_model.txt."""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coarse_cut_model as CC  # noqa: E402

Z, oracle_py = CC.Z, CC.oracle_py
STRIP_W, STRIP_H, BLOCK_W, NC, NF = CC.STRIP_W, CC.STRIP_H, CC.BLOCK_W, CC.NC, CC.NF
M = NC + NF


def _ray(ij):
    """-> (t of the merged fine samples, their densities, first fine sample behind the fine cut)"""
    S = CC._STATE
    d = oracle_py.render_ray_debug(S["nets"][0], S["nets"][1], S["cam"], S["opts"], ij[0], ij[1])
    return (np.asarray(d["t_merged"], np.float32).copy(), np.asarray(d["sigma_fine"], np.float32).copy(),
            CC.first_behind(d["sigma_fine"], d["t_merged"], S["far"]))


def _blocks(a, strips):
    """(strips, 4, 32, ...) per-ray data -> (blocks, 32 rays row-major, ...)"""
    tail = a.shape[3:]
    return a.reshape(strips, STRIP_H, STRIP_W // BLOCK_W, BLOCK_W, *tail).transpose(0, 2, 1, 3, *range(4, 4 + len(tail))).reshape(-1, 32, *tail)


def run(pool, seed, strips):
    rng = np.random.default_rng(seed)
    corners = [(STRIP_W * int(rng.integers(0, 800 // STRIP_W)), STRIP_H * int(rng.integers(0, 800 // STRIP_H))) for _ in range(strips)]
    rays = [(y0 + i, x0 + j) for x0, y0 in corners for i in range(STRIP_H) for j in range(STRIP_W)]
    out = pool.map(_ray, rays, chunksize=32)
    tb = _blocks(np.stack([o[0] for o in out]).reshape(strips, STRIP_H, STRIP_W, M), strips)
    sb = _blocks(np.stack([o[1] for o in out]).reshape(strips, STRIP_H, STRIP_W, M), strips)
    cb = _blocks(np.array([o[2] for o in out]).reshape(strips, STRIP_H, STRIP_W), strips)        # first index behind the cut; M: never cut
    n_blocks, block_tiles = len(tb), 32 * M // 128
    behind = np.arange(M)[None, None, :] >= cb[:, :, None]
    ray, smp = np.repeat(np.arange(32), M), np.tile(np.arange(M), 32)
    skipped = skipped_dense = dense = wholly_behind = 0
    live_samples = live_skipped = 0
    for b in range(n_blocks):
        order = np.lexsort((smp, ray, tb[b].reshape(-1).view(np.uint32)))                        # the order kernel's key
        tile_dense = (sb[b].reshape(-1)[order].reshape(-1, 128) > 0).any(axis=1)
        tile_live = (sb[b].reshape(-1)[order].reshape(-1, 128) > 0).sum(axis=1)
        dense += int(tile_dense.sum())
        live_samples += int(tile_live.sum())
        wholly_behind += int(behind[b].reshape(-1)[order].reshape(-1, 128).all(axis=1).sum())
        if (cb[b] >= M).any():
            continue                                                                             # a ray that is never cut: the block is walked to its end
        position = np.empty(32 * M, np.int64)
        position[order] = np.arange(32 * M)
        last = int((position[np.arange(32) * M + cb[b] - 1] // 128).max())                       # the tile in which the last ray is cut: evaluated
        skipped += block_tiles - 1 - last
        skipped_dense += int(tile_dense[last + 1:].sum())
        live_skipped += int(tile_live[last + 1:].sum())
    tiles = n_blocks * block_tiles
    share = skipped / tiles
    return [f"fine cut: CPU model on {strips} strips of {STRIP_W} x {STRIP_H} pixels = {n_blocks} blocks of 8 x 4 = {32 * n_blocks} rays of the 800x800 view, "
            f"{NC} + {NF} samples, {block_tiles} tiles per block, seed {seed} (tools/fine_cut_model.py)",
            f"strips (x0, y0): {corners}",
            f"  rays the fine network cuts somewhere in near..far                                     {float((cb < M).mean()):.3f}",
            f"  blocks of 8 x 4 all of whose rays are cut                                             {float((cb < M).all(axis=1).mean()):.3f}",
            f"  fine samples behind their own ray's cut (the bound of any mapping)                    {float(behind.mean()):.3f}",
            f"  tiles the block-sequential walk never starts (behind the last ray's cutting tile)     {share:.4f}",
            f"  ... of them all sigma = 0 (the vote skips their colour head already)                  {(skipped - skipped_dense) / tiles:.4f}",
            f"  ... of them with density (trunk and colour head)                                      {skipped_dense / tiles:.4f}   = {skipped_dense / max(skipped, 1):.3f} of the skipped tiles",
            f"  tiles wholly behind their rays' cuts (what the rule could skip at best)               {wholly_behind / tiles:.4f}",
            f"  tiles with density among all tiles                                                    {dense / tiles:.3f}",
            f"  sigma > 0 samples in skipped tiles / all sigma > 0 samples                            {live_skipped / max(live_samples, 1):.3f}", ""], share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", default="0:56,1:56", help="independent draws as seed:strips, 32 x 4-pixel strips of four 8 x 4 blocks each")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(Z.ROOT, "profiles", "finecut_cpu_model.txt"))
    args = ap.parse_args()
    oracle_py.build()
    lines, shares = [], []
    with multiprocessing.Pool(args.jobs, initializer=CC._init) as pool:
        for draw in args.draws.split(","):
            seed, strips = (int(x) for x in draw.split(":"))
            l, share = run(pool, seed, strips)
            lines += l
            shares.append(share)
    lines.append(f"skipped-tile share per draw: {', '.join(f'{s:.4f}' for s in shares)}; mean {np.mean(shares):.4f} -- the expectation the device's "
                 "tiles_skipped / tiles is compared with (not a gate)")
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
