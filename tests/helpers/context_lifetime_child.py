"""Three cycles of {create a Renderer, load the lego networks, one small call of every family that grows a buffer of the context, destroy}
in one process, with the device's free memory read behind each (tests/test_gpu_context_lifetime.py).  Every output of cycles 2 and 3 must
equal cycle 1's bit for bit (raises otherwise).  Prints "free <bytes after cycle 1> <after 2> <after 3>" and exits 0.

torch is imported and initialised BEFORE the library is loaded (see tests/helpers/ray_batch_torch_child.py): its wheel brings its own HIP
runtime, and torch.cuda.mem_get_info is how the free memory is read."""
import json
import os
import sys

import torch

torch.cuda.init()
assert torch.cuda.is_available()

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N  # noqa: E402

SCENE = sys.argv[1]
LO, DIMS = (-1.3, -1.3, -0.8), (16, 16, 16)
STEP = (2.6 / 16, 2.6 / 16, 2.2 / 16)
PLAN = dict(n_coarse=16, fine_samples_per_ray=24, seed=3)


def cycle(samples):
    out = []
    with N.Renderer(0) as r:
        co, fi = r.load_scene(SCENE)
        cam = N.camera_from_samples(samples, 8, 8, 16)
        out.append(N.render_image(co, fi, cam, 24, seed=3))
        out.extend(N.render_image(co, fi, cam, 24, seed=3, ssaa=2, aux=True))
        out.append(N.render_image_rgba8(co, fi, cam, 24, seed=3, alpha="straight"))
        out.append(N.render_image(co, fi, cam, 24, seed=3, skip_dead=True, dtype="bf16x3"))
        out.append(N.render_image(co, fi, cam, 24, seed=3, certify_zero=True))
        dirs = r.stage_ray_dirs(cam, 0, 0, 8, 8).reshape(-1, 3)                     # the stage family
        out.append(dirs)
        origins = np.tile(np.float32(cam.pos), (len(dirs), 1))
        bounds = np.tile(np.float32([cam.near, cam.far]), (len(dirs), 1))
        out.extend(N.render_rays(co, fi, origins, dirs, 0.0, 0.0, bounds=bounds, aux=True, **PLAN))
        out.extend(N.render_rays(co, fi, origins, dirs, 0.0, 0.0, bounds=bounds, aux=True, normals_h=1e-3, **PLAN))
        sigma, bits, count, _ = fi.density_grid(LO, STEP, DIMS, threshold=1.0)
        assert 0 < count < 16 ** 3
        out.extend((sigma, bits))
        for certify in (False, True):
            got = N.render_rays_clipped(co, fi, bits, LO, STEP, DIMS, origins, dirs, 0.0, 0.0, bounds=bounds, aux=True, return_hit=True,
                                        certify_zero=certify, **PLAN)
            assert got[4] > 0                                                      # some rays are rendered, not only filled
            out.extend(got[:4])
        mesh = fi.extract_mesh(LO, STEP, DIMS, 1.0, normals=True, colours=True, keep_largest=1)
        assert len(mesh.triangles) > 0
        out.extend((mesh.vertices, mesh.normals, mesh.colours, mesh.triangles))
        ix = np.indices(DIMS, dtype=np.float32).reshape(3, -1)
        pts = np.ascontiguousarray(np.float32(LO)[:, None] + np.float32(STEP)[:, None] * ix)
        out.append(fi.density_gradient(pts, 1e-3))
        out.extend(fi.forward_batch(pts[:, :256], np.tile(np.float32([0, 0, -1]), (256, 1))))
    return [np.ascontiguousarray(a) for a in out]



def main():
    with open(os.path.join(SCENE, "tf_reference_samples.json")) as f:
        samples = json.load(f)
    first, free = None, []
    for k in range(3):
        out = cycle(samples)
        torch.cuda.synchronize(0)
        free.append(torch.cuda.mem_get_info(0)[0])
        if first is None:
            first = out
            continue
        assert len(out) == len(first)
        for i, (a, b) in enumerate(zip(out, first)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"cycle {k + 1}: output {i} differs from cycle 1's"
    print("free", *free)


main()
