"""tests/helpers/render_restatement.py checked on the CPU, before any GPU test leans on it:

  * with the oracle back end the restatement IS oracle.render_image, bit for bit, in every branch (hierarchical, no resampling
    for n_coarse < 3 or n_fine == 0, coarse-only, SSAA 2 and 3);
  * the probe network (tools/scene_utils.random_scene(root, 11, view_gain=8.0), 12 x 12 camera, 20 + 50 samples, seed 3) makes a
    single sample per ray that took its NEIGHBOUR's view direction visible at Gate 1 on a quarter of the pixels or more -- on
    lego such a mutant moves a pixel by 1e-6 and no composited-pixel check can see it;
  * random_scene without view_gain still writes the files it wrote before the keyword existed."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import SCENE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import render_restatement as RR  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# lego windows on the model's silhouette at that sample count (white and non-white pixels), origins no multiple of anything; with two
# or three samples per ray most rays miss the model, so those shapes look at the middle of the 256 x 256 frame
@pytest.mark.parametrize("W,nc,nf,crop,kw", [
    (96, 64, 128, (19, 55, 7, 5), {}),
    (96, 20, 50, (17, 53, 8, 6), {}),
    (256, 3, 5, (121, 100, 7, 5), {}),
    (256, 2, 5, (121, 100, 7, 5), {}),               # n_coarse < 3: no resampling, the fine network on the coarse samples
    (96, 33, 0, (19, 55, 7, 5), {}),                 # n_fine == 0: the same branch
    (96, 64, 0, (19, 55, 7, 5), dict(coarse_only=True)),
    (96, 20, 50, (22, 56, 4, 3), dict(ssaa=2)),       # 8 x 6 sub-rays
    (96, 20, 50, (21, 56, 2, 2), dict(ssaa=3)),       # 6 x 6 sub-rays
], ids=["64+128", "20+50", "3+5", "2+5", "33+0", "coarse-only 64", "ssaa 2", "ssaa 3"])
def test_oracle_restatement_is_the_oracle_render(oracle, oracle_nets, samples, W, nc, nf, crop, kw):
    cam = oracle.camera_from_samples(samples, W, W)
    seed = 2 ** 40 + 7
    want = oracle.render_image(*oracle_nets, cam, oracle.make_opts(nc, nf, crop=crop, seed=seed, **kw))
    got = RR.restate(RR.OracleBackend(oracle, *oracle_nets), cam, nc, nf, crop, seed, **kw)
    assert got["image"].shape == want.shape and np.array_equal(_bits(got["image"]), _bits(want))
    white = (want == 1.0).all(axis=2)
    assert white.any() and not white.all()
    n = nc if (kw.get("coarse_only") or nf == 0 or nc < 3) else nc + nf
    R = crop[2] * crop[3] * kw.get("ssaa", 1) ** 2
    assert got["t_fine"].shape == (R, n) and got["rgb_fine"].shape == (R, n, 3) and got["w_fine"].shape == (R, n)
    assert got["t_coarse"].shape == got["sigma_coarse"].shape == (R, nc)


def test_oracle_restatement_per_ray_data_is_the_oracle_debug_dump(oracle, oracle_nets, samples):
    cam = oracle.camera_from_samples(samples, 96, 96)
    x0, y0, w, h = 21, 56, 3, 2
    got = RR.restate(RR.OracleBackend(oracle, *oracle_nets), cam, 20, 50, (x0, y0, w, h), 5)
    for r, (i, j) in enumerate((i, j) for i in range(h) for j in range(w)):
        d = oracle.render_ray_debug(*oracle_nets, cam, oracle.make_opts(20, 50, seed=5), y0 + i, x0 + j)
        for mine, theirs in (("dirs", "dir_hat"), ("t_coarse", "t_coarse"), ("sigma_coarse", "sigma_coarse"), ("t_fine", "t_merged"),
                             ("sigma_fine", "sigma_fine"), ("rgb_fine", "rgb_fine"), ("w_fine", "w_fine")):
            assert np.array_equal(_bits(got[mine][r]), _bits(d[theirs])), (r, mine)
        assert np.array_equal(_bits(got["image"][i, j]), _bits(d["rgb"]))


def test_mutant_hook_changes_only_the_colours_of_the_first_sample(oracle, oracle_nets, samples):
    cam = oracle.camera_from_samples(samples, 96, 96)
    be = RR.OracleBackend(oracle, *oracle_nets)
    a = RR.restate(be, cam, 20, 50, (19, 55, 4, 3), 5)
    b = RR.restate(be, cam, 20, 50, (19, 55, 4, 3), 5, fine_dirs=RR.roll_first_sample)
    for k in ("t_coarse", "sigma_coarse", "t_fine", "sigma_fine", "w_fine"):     # density does not see the direction
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["rgb_fine"][:, 1:], b["rgb_fine"][:, 1:]) and (a["rgb_fine"][:, 0] != b["rgb_fine"][:, 0]).any()


# ---- the probe network ------------------------------------------------------------------------------------------------------------
def _tree_hash(root):
    h = hashlib.sha256()
    for p in sorted(root.rglob("*")):
        if p.is_file():
            h.update(str(p.relative_to(root)).encode())
            h.update(p.read_bytes())
    return h.hexdigest()


def test_random_scene_default_files_are_unchanged(tmp_path):
    """SHA-256 over (relative path, bytes) of every file, recorded from random_scene as it was before view_gain existed."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from scene_utils import random_scene
    assert _tree_hash(random_scene(tmp_path / "a", 11)) == "b21ce6af4a619654f6503297bf499868ad2fb3625735f1781fbe6c1de3881e97"
    assert _tree_hash(random_scene(tmp_path / "b", 7, alpha_bias=(2.0, 2.0), alpha_scale=0.01)) == \
        "387efca885c1bbe542aaf64927255348b4b25f4771d4f2a4f855af94710abfe0"
    assert _tree_hash(random_scene(tmp_path / "c", 11, view_gain=1.0)) == _tree_hash(tmp_path / "a")
    gained = random_scene(tmp_path / "d", 11, view_gain=8.0)
    for which in ("coarse", "fine"):
        for f in sorted((tmp_path / "a" / which).iterdir()):
            a, b = f.read_bytes(), (gained / which / f.name).read_bytes()
            if f.name != "viewdirs_kernel.bin":
                assert a == b, f
                continue
            wa, wb = np.frombuffer(a, "<f4").reshape(283, 128), np.frombuffer(b, "<f4").reshape(283, 128)
            assert np.array_equal(wa[:256], wb[:256]) and np.array_equal(wa[256:] * np.float32(8.0), wb[256:])


def _mutant_shares(oracle, root, ks):
    """Share of the pixels (columns > 0) that move by more than 5e-4 when the first k samples of each ray take the previous ray's
    direction in the fine colour head: the oracle's own per-ray data, re-evaluated and composited by the oracle."""
    samples = oracle.load_samples(os.path.join(SCENE, "tf_reference_samples.json"))
    P = RR.PROBE
    co, fi = oracle.Net(str(root / "coarse")), oracle.Net(str(root / "fine"))
    cam = oracle.camera_from_samples(samples, P["size"], P["size"])
    opts = oracle.make_opts(P["nc"], P["nf"], seed=P["seed"])
    far, o = float(cam.far), np.array(list(cam.pos), np.float32)
    rays = [[oracle.render_ray_debug(co, fi, cam, opts, i, j) for j in range(P["size"])] for i in range(P["size"])]
    moved = {k: [] for k in ks}
    live = []
    for i in range(P["size"]):
        for j in range(1, P["size"]):
            d, prev = rays[i][j], rays[i][j - 1]
            t = d["t_merged"]
            pts = RR.ray_points(o, d["dir_hat"][None], t[None])
            live.append((d["w_fine"] > 0).mean())
            for k in ks:
                dirs = np.repeat(d["dir_hat"][None], len(t), axis=0)
                dirs[:k] = prev["dir_hat"]
                rgb, sg = fi.forward_batch(pts, dirs)
                assert np.array_equal(_bits(sg), _bits(d["sigma_fine"]))
                moved[k].append(np.abs(oracle.integrate_ray(rgb, sg, t, far) - d["rgb"]).max())
    return {k: float((np.array(v) > 5e-4).mean()) for k, v in moved.items()}, float(np.mean(live))


def test_probe_makes_one_misrouted_sample_visible(oracle, tmp_path):
    """Measured (132 pixels, share moved by more than 5e-4):   k = 1    k = 4    k = 8
         view_gain 8 (the probe)                               0.508    0.742    0.841
         view_gain 1 (the same fog, plain random weights)      0.098    0.159    0.303
    (the figures of the issue that asked for this test: 51 / 74 / 84 % and 10 / 16 / 30 %).  61 % of the probe's fine samples have a
    positive density (ReLU zeros elsewhere), none is cut off by the transmittance.
    Asserted: k = 1 on the probe moves at least 25 % of the pixels beyond Gate 1's 5e-4, which allows none."""
    shares, live = _mutant_shares(oracle, RR.probe_scene(tmp_path / "probe"), (1, 4, 8))
    print(f"\nprobe (gain 8): shares above 5e-4: {shares}; live samples {live:.3f}")
    assert shares[1] >= 0.25, shares
    assert shares[1] <= shares[4] <= shares[8]
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from scene_utils import random_scene
    plain, _ = _mutant_shares(oracle, random_scene(tmp_path / "plain", RR.PROBE["scene_seed"]), (1, 4, 8))
    print(f"gain 1: {plain}")
    assert plain[1] < shares[1]                           # the gain is what makes the probe sharp
