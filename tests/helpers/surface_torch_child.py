"""render_rays_device(d_depth_q=, quantiles=) and point_cloud_device on torch tensors, on a torch stream == the host entry points on the
same inputs, in a process of its own (tests/test_gpu_surface.py).

torch is imported and initialised BEFORE the library is loaded, as in ray_batch_torch_child.py (one HIP runtime per process: torch's has
to be the first).  The stream is torch's, not the context's: the clearing of the compaction's state words, the running offset between
passes and the count's read-back all run on it, and the outputs live in torch's allocator.  Prints "ok <n comparisons>" and exits 0, or
raises."""
import os
import sys

import torch

torch.cuda.init()
assert torch.cuda.is_available()

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N  # noqa: E402

QS = (0.25, 0.5, 0.75)


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
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    t_dirs, t_bounds = dev(dirs), dev(bounds)
    stream = torch.cuda.Stream()
    done = 0
    os.environ["NERF_MAX_RAYS_PER_PASS"] = "50"                            # three passes: the running offset crosses two boundaries
    with N.Renderer(0) as r:
        r.load_scene(scene)
        for o, n_origins in ((origins, n), (origins[3], 1)):
            t_o = dev(o)
            kw = dict(n_coarse=nc, seed=9)
            # quantile depths
            for dtype in ("f32", "f16x2"):
                host = N.render_rays(r.coarse, r.fine, o, dirs, 0.0, 0.0, nf, bounds=bounds, dtype=dtype, aux=True, quantiles=QS, **kw)
                assert (host[3][1] != 0).sum() >= 8
                rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
                depth, opacity = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
                depth_q = torch.full((len(QS), n), 7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                st = N.render_rays_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, rgb.data_ptr(),
                                          d_bounds=t_bounds.data_ptr(), dtype=dtype, d_depth=depth.data_ptr(), d_opacity=opacity.data_ptr(),
                                          stream=stream.cuda_stream, d_depth_q=depth_q.data_ptr(), quantiles=QS, **kw)
                assert st is None
                stream.synchronize()
                for got, want in zip((rgb, depth, opacity, depth_q), host):
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), ("quantiles", n_origins, dtype)
                    done += 1
            # point clouds, without and with normals; the count comes back through the device word alone, then through the host count
            for step in (None, h):
                cloud, stats = N.point_cloud(r.coarse, r.fine, o, dirs, 0.0, 0.0, nf, bounds=bounds, min_opacity=0.4, normals_h=step, return_stats=True, **kw)
                m = len(cloud["ray"])
                assert stats.n_passes == 3 and 8 <= m <= n
                for want_count in (False, True):
                    out = {k: torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") for k in ("xyz", "rgb", "normals")}
                    out.update({k: torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for k in ("depth", "opacity")})
                    ray = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    got = N.point_cloud_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, n, out["xyz"].data_ptr(),
                                               out["rgb"].data_ptr(), min_opacity=0.4, normals_h=step,
                                               d_normals=None if step is None else out["normals"].data_ptr(), d_ray=ray.data_ptr(),
                                               d_depth=out["depth"].data_ptr(), d_opacity=out["opacity"].data_ptr(), d_n_points=count.data_ptr(),
                                               d_bounds=t_bounds.data_ptr(), stream=stream.cuda_stream, want_count=want_count, **kw)
                    assert got == (m if want_count else None)
                    stream.synchronize()
                    assert int(count.cpu().numpy()[0]) == m
                    assert np.array_equal(ray.cpu().numpy()[:m].view(np.uint32), cloud["ray"]) and (ray.cpu().numpy()[m:] == -1).all()
                    for k in ("xyz", "rgb", "depth", "opacity") + (("normals",) if step is not None else ()):
                        back = out[k].cpu().numpy()
                        assert np.array_equal(bits(back[:m]), bits(cloud[k])), ("points", k, n_origins, step, want_count)
                        assert (back[m:] == 7.0).all(), ("written behind the records", k)
                        done += 1
                    if step is None:
                        assert (out["normals"].cpu().numpy() == 7.0).all()
    print(f"ok {done}")


if __name__ == "__main__":
    main(sys.argv[1])
