#!/usr/bin/env python3
"""CPU measurement and timing model for zero-step skipping of the f32 MLP kernels (mlp_f32_core.hip.h tile_steps<*, true>).

How often is a k-step of a 256-wide layer dead -- its two hidden units zero after the ReLU for all 32 points of a wave -- on the
benchmark's own workload, and what does skipping its MFMAs buy while the four waves of a workgroup still meet at one barrier per
16-KiB chunk?

  * 320 rays of the 800x800 benchmark view: 40 random row segments of 8 adjacent pixels (seed 0);
  * sample positions from the oracle (render_ray_debug): 64 coarse, 64 + 128 fine per ray, ray-major like the kernels' point order;
  * the trunk restated in numpy (float32), checked against the oracle's sigma;
  * a k-step = register r of input tile t = units 32 t + ROW_OF[r][0 / 1] (mlp_layout.h regFeature) over a wave's 32 points;
  * timing model: a chunk (8 macro-steps) takes as long as its slowest wave; an executed macro-step costs 1, a skipped one SKIP_COST
    (its LDS reads and DMA piece remain) -- an ASSUMPTION, bracketed by 0.10 and 0.25; the encoding tiles of dense0 / dense5 and the
    direction tile are dense;
  * ray grouping (mlp_layout.h ray_group_first_slot): the same wave tiles, but the four waves of a workgroup tile hold the same 32-sample
    segment of four adjacent rays instead of 128 consecutive samples -- the row "grouped: 4 adjacent rays x one segment", at the skip
    cost the MI355X showed (0.28).

Reads only oracle/ and lego_rust/.  Writes profiles/zskip_cpu_model.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_py  # noqa: E402

SCENE = os.path.join(ROOT, "lego_rust")
ROW_OF = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for h in (0, 1)] for r in range(16)])
SKIP_COSTS = (0.10, 0.25)
FRAME_MS, FINE_MS, COARSE_MS = 1149.0, 875.0, 271.0   # profiles/fold_summary.md
SKIP_COST_MEASURED = 0.28                               # the cost that reproduces the measured fine kernel (0.8838 against 0.8835)
ZSKIP_FRAME_MS, ZSKIP_FINE_MS, ZSKIP_COARSE_MS = 1026.0, 769.0, 254.0   # the frame with zero-step skipping, ungrouped


def load(d):
    W = {}
    for line in open(os.path.join(d, "shapes.txt")):
        name, *dims = line.split()
        W[name] = np.fromfile(os.path.join(d, name + ".bin"), dtype="<f4").reshape([int(x) for x in dims])
    return W


def encode(p):
    """63 features: x, y, z, then per octave o = 0..9: sin(2^o p) (3), cos(2^o p) (3)  (src/network.rs:263-292)."""
    out = [p]
    for o in range(10):
        out += [np.sin(np.float32(2.0 ** o) * p), np.cos(np.float32(2.0 ** o) * p)]
    return np.concatenate(out, axis=1).astype(np.float32)


def trunk(W, pts):
    """-> (list of the outputs of dense0..7 after the ReLU, sigma)."""
    e = encode(pts)
    acts, h = [], e
    for i in range(8):
        x = np.concatenate([e, h], axis=1) if i == 5 else h
        h = np.maximum(x @ W[f"dense{i}_kernel"] + W[f"dense{i}_bias"], 0).astype(np.float32)
        acts.append(h)
    return acts, np.maximum(h @ W["alpha_kernel"][:, 0] + W["alpha_bias"][0], 0)


def step_live(act, order=None):
    """act (n, 256), n a multiple of 32 -> live[wave, k-step 0..127]: some lane value of the step's B register is non-zero.  `order`
    permutes the units first (position j of the packed stream holds unit order[j])."""
    if order is not None:
        act = act[:, order]
    nz = (act != 0).reshape(-1, 32, 256).any(axis=1)                 # (wave, unit): live anywhere in the wave's 32 points
    units = np.stack([32 * (st >> 4) + ROW_OF[st & 15] for st in range(128)])   # (128, 2)
    return nz[:, units[:, 0]] | nz[:, units[:, 1]]


def model_time(live_layers, dense_steps, nt4_last, skip_cost):
    """live_layers: per ReLU-input layer live[wave, 128] (waves a multiple of 4) -> time relative to executing every step.
    Chunks of 8 macro-steps (8 k-steps of an 8-tile layer, 16 of the 4-tile viewdirs' layer); per chunk the slowest of the 4 waves."""
    total, full = 0.0, 0.0
    for li, live in enumerate(live_layers):
        cost = np.where(live, 1.0, skip_cost)                           # per k-step, in macro-steps of an 8-tile layer
        if nt4_last and li == len(live_layers) - 1:
            cost = 0.5 * cost.reshape(cost.shape[0], 64, 2).sum(axis=2)  # a macro-step holds two k-steps of 4 MFMAs each
            per_chunk = cost.reshape(cost.shape[0], 8, 8).sum(axis=2)
        else:
            per_chunk = cost.reshape(cost.shape[0], 16, 8).sum(axis=2)
        wg = per_chunk.reshape(-1, 4, per_chunk.shape[1]).max(axis=1)   # barrier per chunk: the slowest wave
        total += wg.sum()
        full += wg.size * 8.0
    n_wg = live_layers[0].shape[0] // 4
    return (total + n_wg * dense_steps) / (full + n_wg * dense_steps)


def group_rays(live, segments):
    """live[wave, 128] in ray-major wave order (wave tile g = ray * segments + segment) -> the same rows in the order the grouped launch
    hands them to (workgroup tile, wave): tile b * segments + j, wave w = segment j of ray 4 b + w.  The ray count is a multiple of 4 here."""
    g = np.arange(live.shape[0]).reshape(-1, 4, segments).transpose(0, 2, 1).reshape(-1)
    return live[g]


def main():
    oracle_py.build(); oracle_py.lib()
    nets = {"coarse": oracle_py.Net(os.path.join(SCENE, "coarse")), "fine": oracle_py.Net(os.path.join(SCENE, "fine"))}
    W = {k: load(os.path.join(SCENE, k)) for k in nets}
    samples = oracle_py.load_samples(os.path.join(SCENE, "tf_reference_samples.json"))
    cam = oracle_py.camera_from_samples(samples, 800, 800)
    opts = oracle_py.make_opts(64, 128, seed=0)
    rng = np.random.default_rng(0)
    origin = np.asarray(samples["camera_origin"], np.float32)
    pts = {"coarse": [], "fine": []}
    sig = {"coarse": [], "fine": []}
    for _ in range(40):
        row, col = int(rng.integers(0, 800)), int(rng.integers(0, 800 - 8))
        for j in range(col, col + 8):
            d = oracle_py.render_ray_debug(nets["coarse"], nets["fine"], cam, opts, row, j)
            for k, t, s in (("coarse", d["t_coarse"], d["sigma_coarse"]), ("fine", d["t_merged"], d["sigma_fine"])):
                pts[k].append((origin[None, :] + d["dir_hat"][None, :] * t[:, None]).astype(np.float32))
                sig[k].append(s)
    lines = ["zero-step skipping: CPU measurement on 320 rays of the 800x800 view + chunk-coupled timing model (tools/zero_step_model.py)", ""]
    ratios, grouping = {}, {}
    for k in ("fine", "coarse"):
        P = np.concatenate(pts[k]); S = np.concatenate(sig[k])
        acts, s = trunk(W[k], P)
        rel = np.abs(s - S).max() / (1 + np.abs(S).max())
        lines.append(f"{k}: {P.shape[0]} points; numpy trunk vs oracle sigma: max |d| / (1 + max |sigma|) = {rel:.1e}")
        # unit orders: as packed; sorted by how often a unit is live on these rays; the same from 4096 uniform points in +-2.5
        box = np.random.default_rng(1).uniform(-2.5, 2.5, size=(4096, 3)).astype(np.float32)
        box_acts, _ = trunk(W[k], box)
        orders = {"as packed": [None] * 8,
                  "sorted, same rays": [np.argsort(-(a != 0).mean(axis=0), kind="stable") for a in acts],
                  "sorted, 4096 uniform points": [np.argsort(-(a != 0).mean(axis=0), kind="stable") for a in box_acts]}
        lines.append(f"  {'output of':10s} {'zeros':>6s} {'dead steps / 32 pts (as packed)':>32s} {'(sorted, same rays)':>20s} {'(sorted, uniform)':>18s}")
        for i, a in enumerate(acts):
            dead = [1.0 - step_live(a, orders[o][i]).mean() for o in orders]
            lines.append(f"  dense{i:<5d} {(a == 0).mean():6.2f} {dead[0]:32.2f} {dead[1]:20.2f} {dead[2]:18.2f}")
        full = k == "fine"
        # ReLU-input layers: dense1..4 (outputs of dense0..3), dense5's h4 part, dense6, dense7, and for the full kernel viewdirs' (dense7's output)
        consumers = list(range(7)) + ([7] if full else [])
        dense_steps = 32 + 32 + (8 if full else 0)      # encoding tiles of dense0 and dense5 (2 x 16 macro-steps each) + the direction tile
        for name, order in orders.items():
            live = [step_live(acts[i], order[i]) for i in consumers]
            r = [model_time(live, dense_steps, full, c) for c in SKIP_COSTS]
            ratios[(k, name)] = r
            ex = np.mean([l.mean() for l in live])
            lines.append(f"  {name:28s}: executed share of ReLU k-steps {ex:.3f}; kernel time x {r[0]:.3f} (skip cost {SKIP_COSTS[0]}) .. {r[1]:.3f} ({SKIP_COSTS[1]})")
        # the same wave tiles handed out in groups: the 320 rays come in runs of 8 adjacent columns = two blocks of four
        live = [step_live(acts[i]) for i in consumers]
        segments = (192 if full else 64) // 32
        grouping[k] = (model_time(live, dense_steps, full, SKIP_COST_MEASURED),
                       model_time([group_rays(l, segments) for l in live], dense_steps, full, SKIP_COST_MEASURED))
        lines.append(f"  skip cost {SKIP_COST_MEASURED} (MI355X): as packed x {grouping[k][0]:.4f}; grouped: 4 adjacent rays x one segment x {grouping[k][1]:.4f}")
        lines.append("")
    lines.append(f"frame (from {FRAME_MS:.0f} ms = {FINE_MS:.0f} fine + {COARSE_MS:.0f} coarse + 3):")
    for name in ("as packed", "sorted, same rays", "sorted, 4096 uniform points"):
        ms = [3.0 + FINE_MS * ratios[("fine", name)][i] + COARSE_MS * ratios[("coarse", name)][i] for i in range(2)]
        lines.append(f"  {name:28s}: {ms[0]:.0f} .. {ms[1]:.0f} ms")
    ms = [3.0 + ZSKIP_FINE_MS * grouping["fine"][i] / grouping["fine"][0] + ZSKIP_COARSE_MS * grouping["coarse"][i] / grouping["coarse"][0] for i in range(2)]
    lines.append(f"ray grouping at skip cost {SKIP_COST_MEASURED} (from {ZSKIP_FRAME_MS:.0f} ms = {ZSKIP_FINE_MS:.0f} fine + {ZSKIP_COARSE_MS:.0f} coarse + 3): as packed {ms[0]:.0f} ms, grouped {ms[1]:.0f} ms")
    out = os.path.join(ROOT, "profiles", "zskip_cpu_model.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
