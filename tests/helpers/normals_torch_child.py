"""render_rays_device(d_normals=...) and density_gradient_device on torch tensors == the host entry points on the same inputs, in a process
of its own (tests/test_gpu_normals.py).

torch is imported and initialised BEFORE the library is loaded, as in ray_batch_torch_child.py (one HIP runtime per process: torch's has
to be the first).  Prints "ok <n comparisons>" and exits 0, or raises."""
import os
import sys

import torch

torch.cuda.init()
assert torch.cuda.is_available()

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def main(scene):
    rng = np.random.default_rng(5)
    n, nc, nf, h = 117, 20, 50, 1e-3
    target = rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32)              # rays from a ring of eyes towards the model
    ang = rng.uniform(0, 2 * np.pi, n)
    origins = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
    dirs = (target - origins).astype(np.float32)                            # not unit: normalised on the device
    bounds = np.stack([rng.uniform(2.0, 3.0, n), rng.uniform(5.0, 6.0, n)], axis=1).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_dirs, t_bounds = dev(dirs), dev(bounds)
    stream = torch.cuda.Stream()
    done = 0
    with N.Renderer(0) as r:
        r.load_scene(scene)
        for o, n_origins in ((origins, n), (origins[3], 1)):
            for dtype in ("f32", "f16x2"):
                host = N.render_rays(r.coarse, r.fine, o, dirs, 0.0, 0.0, nf, n_coarse=nc, bounds=bounds, seed=9, dtype=dtype, aux=True, normals_h=h)
                assert (np.abs(host[3]).sum(axis=1) > 0).any() and np.isfinite(host[3]).all()
                t_o = dev(o)
                rgb, normals = (torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
                depth, opacity = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
                torch.cuda.synchronize()
                st = N.render_rays_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, rgb.data_ptr(), n_coarse=nc,
                                          d_bounds=t_bounds.data_ptr(), seed=9, dtype=dtype, d_depth=depth.data_ptr(), d_opacity=opacity.data_ptr(),
                                          stream=stream.cuda_stream, d_normals=normals.data_ptr(), normals_h=h)
                assert st is None
                stream.synchronize()
                for got, want in zip((rgb, depth, opacity, normals), host):
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n_origins, dtype)
                    done += 1
        pts = rng.uniform(-1.0, 1.0, (3, 1000)).astype(np.float32)
        want = r.fine.density_gradient(pts, h)
        t_pts, grad = dev(pts), torch.full((3, 1000), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.fine.density_gradient_device(t_pts.data_ptr(), grad.data_ptr(), 1000, h, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(bits(grad.cpu().numpy()), bits(want)) and np.abs(want).max() > 0
        done += 1
    print(f"ok {done}")


if __name__ == "__main__":
    main(sys.argv[1])
