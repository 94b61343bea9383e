"""render_rays_device(certify_zero=True) and render_rays_clipped_device(certify_zero=True) on torch tensors == the UNCERTIFIED host calls
on the same rays, in a process of its own (tests/test_gpu_ray_batch_certify.py).

torch is imported and initialised BEFORE the library is loaded, the order of a torch program that adopts the library (see
ray_batch_torch_child.py).  The certified device forms synchronise the stream themselves: the outputs are read WITHOUT a synchronisation
of the caller's.  Prints "ok <n comparisons>" and exits 0, or raises."""
import os
import sys

import torch

torch.cuda.init()
assert torch.cuda.is_available()

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nerf_rs_amd as N  # noqa: E402

LO, DIMS = (-1.3, -1.3, -0.8), (32, 32, 32)
STEP = (2.6 / 32, 2.6 / 32, 2.2 / 32)


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
            t_o = dev(o)
            for dtype in ("f32", "bf16x3"):
                host = N.render_rays(r.coarse, r.fine, o, dirs, 0.0, 0.0, nf, n_coarse=nc, bounds=bounds, rng_index=idx, seed=9, dtype=dtype, aux=True)
                assert not (host[0] == 1.0).all() and np.isfinite(host[0]).all()
                rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
                depth, opacity = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
                torch.cuda.synchronize()
                st = N.render_rays_device(r.coarse, r.fine, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 0.0, 0.0, nf, rgb.data_ptr(), n_coarse=nc,
                                          d_bounds=t_bounds.data_ptr(), d_rng_index=t_idx.data_ptr(), seed=9, dtype=dtype, d_depth=depth.data_ptr(),
                                          d_opacity=opacity.data_ptr(), stream=stream.cuda_stream, certify_zero=True, return_stats=(dtype == "f32"))
                assert (st is None) == (dtype != "f32")
                if st is not None:
                    assert st.n_rays == n and st.n_certify_violations == 0 and 0 < st.n_exec_fine_trunk < st.n_fine_points
                assert stream.query()                                           # the call has synchronised the stream
                for got, want in zip((rgb, depth, opacity), host):
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (n_origins, dtype)
                    done += 1
        # clipped + certified, per-ray origins
        _, raw, _, _ = r.fine.density_grid(LO, STEP, DIMS, threshold=1.0, want_sigma=False)
        grown = N.dilate_occupancy(r, raw, DIMS, 1)
        t_grown, t_o = dev(grown.view(np.int32)), dev(origins)
        host = N.render_rays_clipped(r.coarse, r.fine, grown, LO, STEP, DIMS, origins, dirs, 2.0, 6.0, nf, n_coarse=nc, rng_index=idx, seed=9, return_hit=True)
        rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        hits = N.render_rays_clipped_device(r.coarse, r.fine, t_grown.data_ptr(), LO, STEP, DIMS, t_o.data_ptr(), n, t_dirs.data_ptr(), n, 2.0, 6.0, nf,
                                            rgb.data_ptr(), n_coarse=nc, d_rng_index=t_idx.data_ptr(), seed=9, stream=stream.cuda_stream, certify_zero=True)
        assert stream.query() and hits == host[2] and 0 < hits < n
        done += 1
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(host[0]))
        done += 1
    print(f"ok {done}")


if __name__ == "__main__":
    main(sys.argv[1])
