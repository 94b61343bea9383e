#!/usr/bin/env python3
"""Generate tests/golden/aux_c3_800.npz: expected-depth and opacity maps from the CPU oracle (oracle/nerf_oracle.c).

Per ray, from render_ray_debug's exact fine weights w_fine and merged sample positions t_merged (the definitions
in include/nerf_mi355x.h, nerf_render_image_aux):
    opacity = sum_i w_i          summed in sample order in f32
    depth   = sum_i (t_i * w_i)  summed in sample order in f32, separate multiply and add
Two 64x64 crops of the C3 geometry (800x800, 64 + 128 samples, seed 0): the existing colour crop (its rgb is asserted
equal, bit for bit, to crop_c3_800_64_128.npz) and one that straddles the lego silhouette.  make_golden.py is not
touched.  About 70 s per crop on one core; the rays are spread over a process pool.

    python tests/golden/make_golden_aux.py     # rewrites tests/golden/aux_c3_800.npz
"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_py as O  # noqa: E402

SCENE = os.path.join(ROOT, "lego_rust")
OUT = os.path.join(ROOT, "tests", "golden")
CROPS = {"centre": (368, 352, 64, 64), "silhouette": (544, 448, 64, 64)}  # (x0, y0, w, h) in the 800x800 frame
N_COARSE, N_FINE, SEED = 64, 128, 0

_state = {}


def _init():
    S = O.load_samples(os.path.join(SCENE, "tf_reference_samples.json"))
    _state["cam"] = O.camera_from_samples(S, 800, 800)
    _state["co"], _state["fi"] = O.Net(os.path.join(SCENE, "coarse")), O.Net(os.path.join(SCENE, "fine"))
    _state["opts"] = O.make_opts(N_COARSE, N_FINE, seed=SEED)


def ray_maps(ij):
    d = O.render_ray_debug(_state["co"], _state["fi"], _state["cam"], _state["opts"], ij[0], ij[1])
    w, t = d["w_fine"], d["t_merged"]  # zero-padded past nc + n_new: adding +0 changes nothing
    depth = np.float32(0.0); acc = np.float32(0.0)
    for i in range(len(w)):
        depth = np.float32(depth + np.float32(t[i] * w[i]))
        acc = np.float32(acc + w[i])
    return d["rgb"], depth, acc


def render_crop(pool, crop):
    x0, y0, cw, ch = crop
    rays = [(i, j) for i in range(y0, y0 + ch) for j in range(x0, x0 + cw)]  # (row, column), row-major
    res = pool.map(ray_maps, rays, chunksize=32)
    rgb = np.stack([r[0] for r in res]).reshape(ch, cw, 3)
    depth = np.array([r[1] for r in res], np.float32).reshape(ch, cw)
    acc = np.array([r[2] for r in res], np.float32).reshape(ch, cw)
    return rgb, depth, acc


def main():
    out = {"seed": np.uint64(SEED), "n_coarse": N_COARSE, "n_fine": N_FINE, "width": 800, "height": 800}
    with mp.Pool(min(os.cpu_count() or 1, 16), initializer=_init) as pool:
        for name, crop in CROPS.items():
            rgb, depth, acc = render_crop(pool, crop)
            out[f"{name}_crop"] = np.array(crop)
            out[f"{name}_rgb"], out[f"{name}_depth"], out[f"{name}_opacity"] = rgb, depth, acc
            print(f"{name} {crop}: opacity <0.01 {np.mean(acc < 0.01):.3f}, >0.99 {np.mean(acc > 0.99):.3f}, "
                  f"between {np.mean((acc >= 0.01) & (acc <= 0.99)):.3f}; depth max {depth.max():.4f}")
    ref = np.load(os.path.join(OUT, "crop_c3_800_64_128.npz"))
    assert tuple(ref["crop"]) == CROPS["centre"]
    assert np.array_equal(out["centre_rgb"], ref["image"]), "per-ray oracle colour differs from the crop fixture"
    acc = out["silhouette_opacity"]
    assert np.mean(acc < 0.01) >= 0.10 and np.mean(acc > 0.99) >= 0.10, "silhouette crop misses background or solid"
    assert np.mean((acc >= 0.01) & (acc <= 0.99)) >= 0.01, "silhouette crop has too few partial pixels"
    S = O.load_samples(os.path.join(SCENE, "tf_reference_samples.json"))
    out["far"] = np.float32(S["far"]); out["near"] = np.float32(S["near"])
    np.savez_compressed(os.path.join(OUT, "aux_c3_800.npz"), **out)
    print("done ->", os.path.join(OUT, "aux_c3_800.npz"))


if __name__ == "__main__":
    main()
