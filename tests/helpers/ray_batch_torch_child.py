"""render_rays_device on torch tensors == render_rays on the same rays, in a process of its own (tests/test_gpu_ray_batch.py).

torch is imported and initialised BEFORE the library is loaded, the order of a torch program that adopts the library: a torch wheel
brings its own HIP runtime, and a process holds one runtime only if torch's is the first to load (the library's libamdhip64.so.7 then
resolves to it).  Prints "ok <n comparisons>" and exits 0, or raises."""
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
    n, nc, nf = 117, 20, 50
    target = rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32)              # rays from a ring of eyes towards the model
    ang = rng.uniform(0, 2 * np.pi, n)
    origins = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
    dirs = (target - origins).astype(np.float32)                            # not unit: normalised on the device
    bounds = np.stack([rng.uniform(2.0, 3.0, n), rng.uniform(5.0, 6.0, n)], axis=1).astype(np.float32)
    idx = (np.arange(n, dtype=np.uint32) * 7 + 5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t_dirs, t_bounds, t_idx = dev(dirs), dev(bounds), dev(idx.astype(np.int32))
    stream = torch.cuda.Stream()
    done = 0
    with N.Renderer(0) as r:
        r.load_scene(scene)
        for o, n_origins in ((origins, n), (origins[3], 1)):
            for dtype in ("f32", "bf16x3"):
                host = N.render_rays(r.coarse, r.fine, o, dirs, 0.0, 0.0, nf, n_coarse=nc, bounds=bounds, rng_index=idx, seed=9, dtype=dtype, aux=True)
                assert not (host[0] == 1.0).all() and np.isfinite(host[0]).all()
                t_o = dev(o)
                rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
                depth, opacity = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
                torch.cuda.synchronize()
                st = N.render_rays_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, rgb.data_ptr(), n_coarse=nc,
                                          d_bounds=t_bounds.data_ptr(), d_rng_index=t_idx.data_ptr(), seed=9, dtype=dtype, d_depth=depth.data_ptr(),
                                          d_opacity=opacity.data_ptr(), stream=stream.cuda_stream)
                assert st is None
                stream.synchronize()
                for got, want in zip((rgb, depth, opacity), host):
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n_origins, dtype)
                    done += 1
                # colour alone, with the stats: the call synchronises the stream itself
                rgb.fill_(7.0)
                st = N.render_rays_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, rgb.data_ptr(), n_coarse=nc,
                                          d_bounds=t_bounds.data_ptr(), d_rng_index=t_idx.data_ptr(), seed=9, dtype=dtype, stream=stream.cuda_stream,
                                          return_stats=True)
                assert st.n_rays == n and np.array_equal(bits(rgb.cpu().numpy()), bits(host[0]))
                done += 1
    print(f"ok {done}")


if __name__ == "__main__":
    main(sys.argv[1])
