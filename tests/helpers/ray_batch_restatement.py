"""A ray-batch render (render_rays) restated from the public stage calls, on render_restatement's two back ends.

render_rays takes the rays themselves: per-ray origin, direction, [near, far] and RNG index.  restate_rays() makes the same outputs from
calls a host can make one stage at a time and returns every per-ray intermediate (the contract: include/nerf_mi355x.h, "ray batches"):

  1. d = dirs[r], or oracle.normalize(dirs[r]) -- Vec3::normalize, which DESIGN section 2 records as bit-identical to the device's;
  2. t_coarse = oracle.stratified_samples(seed, rng_index[r], near_r, far_r, nc): there is no stage call that takes an index per
     ray, and DESIGN section 2 records the oracle's samples as the device's, bit for bit (tests/test_gpu_sampling_shapes.py holds it);
  3. points fl(o_r + fl(d t)) on the host (render_restatement.ray_points, one ray at a time: the origin is the ray's own);
  4. the coarse network at those points, the ray's direction per sample (arithmetic: render_restatement.pass_dtypes);
  5. resample + merge + sort through the back end, which takes ONE far per call: the rays are grouped by their far value
     (skipped when n_fine == 0 or n_coarse < 3 or coarse_only, as in an image render);
  6. the fine network at the merged points;
  7. integrate_ray through the back end, grouped by far likewise; depth = sum_i (t_i * w_i) and opacity = sum_i w_i from the returned
     weights, in sample order in float32, multiply and add rounded separately (nerf_render_image_aux's definition); with a background
     B the colour is (sum_i w_i c_i) + B * (1 - opacity) from the same weights (nerf_render_image_rgba8's opaque arithmetic).
Nothing here looks at a rendered batch."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_restatement as RR  # noqa: E402


def _groups(values):
    """[(value, indices)] of the distinct float32 values, in order of first appearance."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    seen = {}
    for i, b in enumerate(bits):
        seen.setdefault(int(b), []).append(i)
    return [(float(np.array([b], np.uint32).view(np.float32)[0]), np.array(idx)) for b, idx in seen.items()]


def sums_from_weights(rgb, w, t, background=None):
    """(colour over the background, depth, opacity) from per-sample colours (R, n, 3), weights and positions (R, n): sequential float32
    sums in sample order, every multiply and add rounded on its own (k_composite's walk)."""
    R, n = w.shape
    c = np.zeros((R, 3), np.float32)
    acc = np.zeros(R, np.float32)
    dep = np.zeros(R, np.float32)
    for i in range(n):
        wi = w[:, i].astype(np.float32)
        c = c + rgb[:, i, :].astype(np.float32) * wi[:, None]
        acc = acc + wi
        dep = dep + t[:, i].astype(np.float32) * wi
    bg = np.ones(3, np.float32) if background is None else np.asarray(background, np.float32)
    return (c + bg[None, :] * (np.float32(1.0) - acc)[:, None]).astype(np.float32), dep, acc


def restate_rays(backend, origins, dirs, near, far, bounds, rng_index, nc, nf, seed, coarse_only, dtype, fine_dirs=None, normalize=False,
                 background=None, group_by_far=True):
    """What render_rays(origins, dirs, near, far, nf, n_coarse=nc, bounds=bounds, rng_index=rng_index, seed=seed, ...) computes.

    origins (3,) or (R, 3); dirs (R, 3); bounds None or (R, 2); rng_index None (ray r draws from r) or (R,).
    -> dict: rgb (R, 3), depth, opacity (R,); dirs (R, 3) as the networks saw them; t_coarse, sigma_coarse (R, nc); t_fine, sigma_fine,
    w_fine (R, n), rgb_fine (R, n, 3), pts_fine (3, R * n) as render_restatement.restate returns them; far (R,).
    fine_dirs: render_restatement's mutant hook.  group_by_far=False calls the back end once per ray (what the grouping must equal)."""
    import oracle_py as O
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    R = len(dirs)
    o = np.ascontiguousarray(origins, np.float32)
    o = np.repeat(o[None, :], R, axis=0) if o.ndim == 1 else o
    assert o.shape == (R, 3)
    if normalize:
        dirs = np.stack([O.normalize(d) for d in dirs])
    b = np.ascontiguousarray(bounds, np.float32) if bounds is not None else np.repeat(np.array([[near, far]], np.float32), R, axis=0)
    assert b.shape == (R, 2)
    idx = np.arange(R, dtype=np.uint32) if rng_index is None else np.ascontiguousarray(rng_index, np.uint32)
    dt_coarse, dt_fine = RR.pass_dtypes(dtype, coarse_only)
    t_coarse = np.stack([O.stratified_samples(seed, int(idx[r]), float(b[r, 0]), float(b[r, 1]), nc) for r in range(R)])
    groups = _groups(b[:, 1]) if group_by_far else [(float(b[r, 1]), np.array([r])) for r in range(R)]

    def run(which, t, dt, hook):
        n = t.shape[1]
        per_sample = np.repeat(dirs[:, None, :], n, axis=1)
        if hook is not None:
            per_sample = np.ascontiguousarray(hook(per_sample.copy()), dtype=np.float32)
        pts = np.ascontiguousarray(np.hstack([RR.ray_points(o[r], dirs[r:r + 1], t[r:r + 1]) for r in range(R)]))
        rgb, sigma = backend.forward(which, pts, per_sample.reshape(-1, 3), dt)
        return pts, rgb.reshape(R, n, 3), sigma.reshape(R, n)

    pts_c, rgb_c, sigma_coarse = run(0, t_coarse, dt_coarse, fine_dirs if coarse_only else None)
    if coarse_only:
        t_fine, pts_f, rgb_f, sigma_f = t_coarse, pts_c, rgb_c, sigma_coarse
    else:
        t_fine = t_coarse
        if nf > 0 and nc >= 3:
            t_fine = np.empty((R, nc + nf), np.float32)
            for f, rows in groups:
                t_fine[rows] = backend.resample(t_coarse[rows], sigma_coarse[rows], nf, f, seed, idx[rows])
        pts_f, rgb_f, sigma_f = run(1, t_fine, dt_fine, fine_dirs)
    white = np.empty((R, 3), np.float32)
    w_fine = np.empty(t_fine.shape, np.float32)
    for f, rows in groups:
        img, w = backend.integrate(rgb_f[rows], sigma_f[rows], t_fine[rows], f)
        white[rows], w_fine[rows] = np.asarray(img, np.float32).reshape(-1, 3), w
    rgb, depth, opacity = sums_from_weights(rgb_f, w_fine, t_fine, background)
    if background is None:      # the host sums restate the back end's own compositing: the colour is integrate_ray's, bit for bit
        assert np.array_equal(rgb.view(np.uint32), white.view(np.uint32))
    return dict(rgb=rgb, depth=depth, opacity=opacity, dirs=dirs, t_coarse=t_coarse, sigma_coarse=sigma_coarse, t_fine=t_fine,
                sigma_fine=sigma_f, rgb_fine=rgb_f, w_fine=w_fine, pts_fine=pts_f, far=b[:, 1].copy())


def camera_batch(backend, cam, crop):
    """The batch that is a camera window: (origin (3,), unit dirs (R, 3), near, far, rng_index (R,)) -- rng_index = row * nx + col."""
    x0, y0, w, h = crop
    W, origin, near, far = backend.geometry(cam)
    return origin, backend.ray_dirs(cam, x0, y0, w, h), near, far, RR.pixel_indices(W, x0, y0, w, h)


# ---- the batch no camera can make ---------------------------------------------------------------------------------------------------
DISPLACED = dict(W=800, crop=(311, 287, 13, 9), nc=20, nf=50, seed=2 ** 40 + 7, pairs=((2.0, 6.0), (2.5, 5.5), (3.0, 5.0)))


def displaced_batch(backend, cam, crop, pairs=DISPLACED["pairs"]):
    """A lego window's rays with ray r's origin displaced by 0.05 * ((r mod 7) - 3) along the camera's right vector and its bounds
    cycling through `pairs` (inside the scene's [2, 6]) -> (origins (R, 3), unit dirs (R, 3), bounds (R, 2)); rng_index is left to the
    default (ray r draws from r)."""
    x0, y0, w, h = crop
    _, origin, _, _ = backend.geometry(cam)
    dirs = backend.ray_dirs(cam, x0, y0, w, h)
    R = len(dirs)
    fwd, up = np.asarray(cam.dir, np.float64), np.asarray(cam.up, np.float64)
    right = np.cross(fwd, up)
    right = (right / np.linalg.norm(right)).astype(np.float32)
    shift = (np.float32(0.05) * ((np.arange(R) % 7) - 3).astype(np.float32))
    origins = (origin[None, :] + shift[:, None] * right[None, :]).astype(np.float32)
    bounds = np.array([pairs[r % len(pairs)] for r in range(R)], np.float32)
    return origins, dirs, bounds
