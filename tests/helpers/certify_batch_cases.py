"""Inputs of tests/test_gpu_ray_batch_certify.py: a camera's rays as a batch, a displaced batch no camera can make, and the two network
recipes on which certify_zero's retry loop has work to do (those of tests/test_gpu_certify.py's hot-network tests).  NumPy only."""
import os
import shutil

import numpy as np

F = np.float32


def camera_batch(renderer, cam, W):
    """-> (origin (3,), unit dirs (W*W, 3), near, far, rng_index = row * nx + col) of a W x W camera."""
    dirs = renderer.stage_ray_dirs(cam, 0, 0, W, W, normalize=True).reshape(-1, 3)
    return np.asarray(cam.pos, F).copy(), dirs, float(cam.near), float(cam.far), np.arange(W * W, dtype=np.uint32)


def displace(origin, dirs, near, far, seed=11):
    """Every ray's origin moved by its own amount ALONG the ray (s_r in [-0.6, 0.9]) and ACROSS it (up to 0.05 along a direction
    perpendicular to the ray), its bounds shifted by -s_r to match: the rays still look at the model, each from its own origin over its
    own interval.  -> (origins (n, 3), bounds (n, 2)), float32."""
    rng = np.random.default_rng(seed)
    n = len(dirs)
    d = dirs.astype(np.float64)
    s = rng.uniform(-0.6, 0.9, n)
    helper = np.where(np.abs(d[:, 2:3]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    side = np.cross(d, helper)
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    origins = (np.asarray(origin, np.float64)[None, :] + d * s[:, None] + side * rng.uniform(-0.05, 0.05, n)[:, None]).astype(F)
    bounds = np.stack([near - s, far - s], axis=1).astype(F)
    assert (bounds[:, 1] > bounds[:, 0]).all()
    return origins, bounds


def scaled_lego(scene, root, scale):
    """The lego networks with dense7 (kernel and bias) of both scaled: every density pre-activation (but for the alpha bias) and the
    16-bit pass's errors grow by that factor -- the shipped margins are too tight."""
    for which in ("coarse", "fine"):
        shutil.copytree(os.path.join(scene, which), os.path.join(root, which))
        for t in ("dense7_kernel", "dense7_bias"):
            f = os.path.join(root, which, f"{t}.bin")
            (np.fromfile(f, "<f4") * F(scale)).astype("<f4").tofile(f)
    return root


def beyond_f16_lego(scene, root):
    """dense0 x 2000, dense1 x 50: activations beyond 65 504 -- the f16 pre-filter leaves its range, the bf16 one takes over."""
    for which in ("coarse", "fine"):
        shutil.copytree(os.path.join(scene, which), os.path.join(root, which))
        for t, k in (("dense0_kernel", 2000.0), ("dense0_bias", 2000.0), ("dense1_kernel", 50.0), ("dense1_bias", 50.0)):
            f = os.path.join(root, which, f"{t}.bin")
            (np.fromfile(f, "<f4") * F(k)).astype("<f4").tofile(f)
    return root
