"""A render restated from the public stage calls: one restatement, two back ends.

render_image composes ray directions, stratified samples, the coarse network, resampling, the fine network and compositing inside
one call; restate() makes the same image from the calls a host can make itself, one stage at a time, and hands back every per-ray
intermediate.  The steps (reference: render_block, src/lib.rs:353-472; oracle/nerf_oracle.c render_rays; nerf_render.cpp render_passes):

  1. unit ray directions of the window's rays;
  2. stratified t, RNG pixel_index = (y0 + i) * W + x0 + j in the ray grid;
  3. points o + d * t on the host in float32, the multiply and the add rounded separately (src/lib.rs:396; mlp_common.hip.h
     forms ray-mode points with __fadd_rn(__fmul_rn(...)) for the same reason);
  4. the coarse network's densities at those points, the ray's direction repeated per sample;
  5. resample + merge + sort (skipped -- the fine network then runs on the coarse samples -- when n_fine == 0 or n_coarse < 3:
     sample_importance returns nothing, src/lib.rs:295-297; nerf_render.cpp fine_samples);
  6. the fine network at the merged points;
  7. integrate_ray.
coarse_only composites the coarse network's colours after step 4 (oracle/nerf_oracle.c "if (R->coarse_only)"; nerf_render.cpp
render_passes "if (j.coarse_only)").  ssaa = S renders the window (S x0, S y0, S w, S h) of the camera with S times the pixels per side and
reduces every S x S block of sub-rays by a row-major f32 sum followed by ONE multiply by 1 / S^2 (oracle_render_image "acc * inv";
k_box_downsample).

Which arithmetic runs which pass (nerf_render.cpp plan_job, dtype_coarse): f32 and bf16 renders run both networks in their own arithmetic;
bf16x3 and f16x2 renders take their sample positions from the exact-f32 coarse pass and run only the colour-producing pass in the
split arithmetic (so a coarse_only render runs the coarse network in the split arithmetic).

The two back ends expose the same five operations; OracleBackend is the CPU oracle (oracle_py), GpuBackend the product's stage entry
points and Network.forward_batch.  Nothing here looks at a rendered image: the restatement is independent of the fused path."""
import ctypes

import numpy as np


def pass_dtypes(dtype, coarse_only):
    """(arithmetic of the coarse pass, arithmetic of the fine pass) of a render in `dtype` (nerf_render.cpp plan_job, dtype_coarse)."""
    split = dtype in ("bf16x3", "f16x2")
    return ("f32" if split and not coarse_only else dtype), dtype


def ray_points(origin, dirs, t):
    """(R, 3) unit directions, (R, n) distances -> SoA points (3, R * n) float32: fl(o + fl(d * t))."""
    o = np.asarray(origin, np.float32)
    d = np.asarray(dirs, np.float32)
    prod = d[:, None, :] * np.asarray(t, np.float32)[:, :, None]           # float32 * float32: one rounding
    pts = (o[None, None, :] + prod).astype(np.float32)                     # float32 + float32: the second
    return np.ascontiguousarray(pts.reshape(-1, 3).T)


def pixel_indices(W, x0, y0, w, h):
    return ((y0 + np.arange(h))[:, None] * W + (x0 + np.arange(w))[None, :]).reshape(-1).astype(np.uint32)


def _scaled(c_struct, s):
    """The camera on the ray grid: the same struct with s times the pixels per side (make_rctx; make_raygen)."""
    out = type(c_struct)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(c_struct), ctypes.sizeof(out))
    out.nx, out.ny = c_struct.nx * s, c_struct.ny * s
    return out


class OracleBackend:
    """cam: oracle_py.Camera."""

    def __init__(self, oracle, coarse, fine):
        self.o, self.nets = oracle, (coarse, fine)

    def scaled(self, cam, s):
        return _scaled(cam, s)

    def geometry(self, cam):
        return cam.nx, np.array(list(cam.pos), np.float32), float(cam.near), float(cam.far)

    def ray_dirs(self, cam, x0, y0, w, h):
        return np.stack([self.o.normalize(self.o.get_ray_dir(cam, y0 + i, x0 + j)) for i in range(h) for j in range(w)])

    def stratified(self, cam, x0, y0, w, h, count, seed):
        near, far = float(cam.near), float(cam.far)
        return np.stack([self.o.stratified_samples(seed, int(p), near, far, count) for p in pixel_indices(cam.nx, x0, y0, w, h)])

    def forward(self, which, pts, dirs, dtype):
        if dtype != "f32":
            raise ValueError("the oracle back end restates the reference arithmetic only")
        return self.nets[which].forward_batch(pts, dirs)

    def resample(self, t, sigma, nf, far, seed, pix):
        out = []
        for r in range(len(t)):
            w = self.o.compute_weights(sigma[r], t[r], far)
            new = self.o.sample_importance(seed, int(pix[r]), t[r], w, nf)
            assert len(new) == nf
            out.append(self.o.sort_ascending(np.concatenate([t[r], new])))
        return np.stack(out)

    def integrate(self, rgb, sigma, t, far):
        img = np.stack([self.o.integrate_ray(rgb[r], sigma[r], t[r], far) for r in range(len(t))])
        return img, np.stack([self.o.compute_weights(sigma[r], t[r], far) for r in range(len(t))])


class GpuBackend:
    """cam: nerf_rs_amd Camera; renderer: a Renderer with both networks loaded."""

    def __init__(self, native, renderer):
        self.n, self.r = native, renderer
        self.nets = (renderer.coarse, renderer.fine)

    def scaled(self, cam, s):
        return self.n.Camera(_scaled(cam.c, s), cam.samples_per_ray)

    def geometry(self, cam):
        return cam.nx, cam.pos, float(cam.near), float(cam.far)

    def ray_dirs(self, cam, x0, y0, w, h):
        return self.r.stage_ray_dirs(cam, x0, y0, w, h).reshape(-1, 3)

    def stratified(self, cam, x0, y0, w, h, count, seed):
        return self.r.stage_stratified(cam, x0, y0, w, h, count, seed=seed).reshape(-1, count)

    def forward(self, which, pts, dirs, dtype):
        return self.nets[which].forward_batch(pts, dirs, dtype=dtype)

    def resample(self, t, sigma, nf, far, seed, pix):
        return self.r.stage_resample(t, sigma, nf, far, seed=seed, pixel_index=pix)["t_fine"]

    def integrate(self, rgb, sigma, t, far):
        return self.r.stage_integrate(rgb, sigma, t, far)


def box_reduce(rays, s):
    """(s h, s w, 3) sub-ray colours -> (h, w, 3): row-major f32 sum over each s x s block, then one multiply by 1 / s^2."""
    acc = np.zeros((rays.shape[0] // s, rays.shape[1] // s, 3), np.float32)
    for di in range(s):
        for dj in range(s):
            acc = acc + rays[di::s, dj::s]
    return acc * (np.float32(1.0) / np.float32(s * s))


def restate(backend, cam, nc, nf, crop, seed, coarse_only=False, ssaa=1, dtype="f32", fine_dirs=None):
    """The image render_image(cam, nc + nf, crop, seed, ...) computes, from the back end's stage calls, and its per-ray data.

    -> dict: image (h, w, 3); dirs (R, 3); t_coarse, sigma_coarse (R, nc); t_fine, sigma_fine, w_fine (R, n), rgb_fine (R, n, 3): the
    composited samples and what the colour-producing network returned there (coarse_only: the coarse samples, n = nc; no
    resampling: n = nc; else n = nc + nf); pts_fine (3, R * n): the points that network was given.  R = the window's rays (sub-rays
    with ssaa), row-major.

    fine_dirs: None, or a function (R, n, 3) -> (R, n, 3) applied to the per-sample directions of the colour-producing pass -- the
    hook by which a test builds a MUTANT restatement (a sample given another ray's direction) to show that its assertions bite."""
    s = max(int(ssaa), 1)
    x0, y0, w, h = crop
    rcam = backend.scaled(cam, s) if s > 1 else cam
    X0, Y0, RW, RH = x0 * s, y0 * s, w * s, h * s
    W, origin, _, far = backend.geometry(rcam)
    dt_coarse, dt_fine = pass_dtypes(dtype, coarse_only)
    dirs = backend.ray_dirs(rcam, X0, Y0, RW, RH)
    R = len(dirs)
    pix = pixel_indices(W, X0, Y0, RW, RH)
    t_coarse = backend.stratified(rcam, X0, Y0, RW, RH, nc, seed)

    def run(which, t, dt, hook):
        n = t.shape[1]
        per_sample = np.repeat(dirs[:, None, :], n, axis=1)
        if hook is not None:
            per_sample = np.ascontiguousarray(hook(per_sample.copy()), dtype=np.float32)
        pts = ray_points(origin, dirs, t)
        rgb, sigma = backend.forward(which, pts, per_sample.reshape(-1, 3), dt)
        return pts, rgb.reshape(R, n, 3), sigma.reshape(R, n)

    pts_c, rgb_c, sigma_coarse = run(0, t_coarse, dt_coarse, fine_dirs if coarse_only else None)
    if coarse_only:
        t_fine, pts_f, rgb_f, sigma_f = t_coarse, pts_c, rgb_c, sigma_coarse
    else:
        resampled = nf > 0 and nc >= 3
        t_fine = backend.resample(t_coarse, sigma_coarse, nf, far, seed, pix) if resampled else t_coarse
        pts_f, rgb_f, sigma_f = run(1, t_fine, dt_fine, fine_dirs)
    rays, w_fine = backend.integrate(rgb_f, sigma_f, t_fine, far)
    rays = np.asarray(rays, np.float32).reshape(RH, RW, 3)
    image = box_reduce(rays, s) if s > 1 else rays
    return dict(image=image, dirs=dirs, t_coarse=t_coarse, sigma_coarse=sigma_coarse, t_fine=t_fine, sigma_fine=sigma_f,
                rgb_fine=rgb_f, w_fine=w_fine, pts_fine=pts_f)


def roll_first_sample(per_sample):
    """The mutant reference: sample 0 of every ray is given the previous ray's direction (ray 0 the last ray's)."""
    per_sample[:, 0, :] = np.roll(per_sample[:, 0, :], 1, axis=0)
    return per_sample


# ---- the probe network ------------------------------------------------------------------------------------------------------------
PROBE = dict(scene_seed=11, view_gain=8.0, size=12, nc=20, nf=50, seed=3)


def probe_scene(root):
    """random_scene(root, 11, view_gain=8.0): a fog in which every sample is live and colour follows direction strongly; rendered on
    the 12 x 12 JSON camera (neighbouring rays 3.4 degrees apart) with 20 + 50 samples, seed 3."""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from scene_utils import random_scene
    return random_scene(root, PROBE["scene_seed"], view_gain=PROBE["view_gain"])
