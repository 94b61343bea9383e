"""dilate_occupancy_device, clip_rays_device and render_rays_clipped_device on torch tensors == the host entry points on the same grid and
rays, in a process of its own (tests/test_gpu_ray_clip.py).

torch is imported and initialised BEFORE the library is loaded, the order of a torch program that adopts the library (see
tests/helpers/ray_batch_torch_child.py).  Prints "ok <n comparisons>" and exits 0, or raises."""
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
    rng = np.random.default_rng(6)
    n, nc, nf = 117, 16, 24
    target = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)              # rays from a ring of eyes towards and beside the model
    ang = rng.uniform(0, 2 * np.pi, n)
    origins = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, n)], axis=1).astype(np.float32)
    dirs = (target - origins).astype(np.float32)                            # not unit: normalised on the device
    idx = (np.arange(n, dtype=np.uint32) * 7 + 5)
    bg = (0.5, 0.25, 0.75)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    done = 0
    with N.Renderer(0) as r:
        r.load_scene(scene)
        _, raw, _, _ = r.fine.density_grid(LO, STEP, DIMS, threshold=1.0, want_sigma=False)
        grown, count, bounds = N.dilate_occupancy(r, raw, DIMS, 1, return_stats=True)
        t_raw, t_grown = dev(raw.view(np.int32)), torch.full((len(raw),), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert N.dilate_occupancy_device(r, t_raw.data_ptr(), DIMS, 1, t_grown.data_ptr(), want_stats=True, stream=stream.cuda_stream) == (count, bounds)
        done += 1
        assert np.array_equal(t_grown.cpu().numpy().view(np.uint32), grown) and count > int(np.unpackbits(raw.view(np.uint8)).sum()) > 0
        done += 1
        t_dirs, t_idx = dev(dirs), dev(idx.astype(np.int32))
        for o, n_origins in ((origins, n), (origins[3], 1)):
            t_o = dev(o)
            want_b, want_h, want_n = N.clip_rays(r, grown, LO, STEP, DIMS, o, dirs, 2.0, 6.0, return_count=True)
            assert 0 < want_n < n
            t_b = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
            t_h = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert N.clip_rays_device(r, t_grown.data_ptr(), LO, STEP, DIMS, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 2.0, 6.0, t_b.data_ptr(),
                                      t_h.data_ptr(), stream=stream.cuda_stream) is None
            stream.synchronize()
            assert np.array_equal(bits(t_b.cpu().numpy()), bits(want_b))
            assert np.array_equal(t_h.cpu().numpy().astype(bool), want_h)
            done += 2
            host = N.render_rays_clipped(r.coarse, r.fine, grown, LO, STEP, DIMS, o, dirs, 2.0, 6.0, nf, n_coarse=nc, rng_index=idx, seed=9, background=bg,
                                         aux=True, return_hit=True)
            assert host[4] == want_n and np.array_equal(host[3], want_h) and (host[0][~want_h] == np.float32(bg)).all()
            rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
            depth, opacity = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
            t_h.fill_(7)
            torch.cuda.synchronize()
            hits = N.render_rays_clipped_device(r.coarse, r.fine, t_grown.data_ptr(), LO, STEP, DIMS, t_o.data_ptr(), n_origins, t_dirs.data_ptr(), n, 2.0,
                                                6.0, nf, rgb.data_ptr(), n_coarse=nc, d_rng_index=t_idx.data_ptr(), seed=9, background=bg,
                                                d_depth=depth.data_ptr(), d_opacity=opacity.data_ptr(), d_hit=t_h.data_ptr(), stream=stream.cuda_stream)
            assert hits == want_n
            stream.synchronize()
            for got, want in zip((rgb, depth, opacity), host):
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), n_origins
                done += 1
            assert np.array_equal(t_h.cpu().numpy().astype(bool), want_h)
            done += 1
    print(f"ok {done}")


if __name__ == "__main__":
    main(sys.argv[1])
