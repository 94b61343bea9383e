"""What the ray-grouping tests share (test_ray_grouping_host.py, test_gpu_ray_grouping.py): the mapping table as the library reports it
(nerf_debug_ray_grouping calls the function the f32 ray-mode kernels call, mlp_layout.h ray_group_first_slot) and what skip_empty must
count under a given table.  Nothing here needs a GPU."""
import ctypes as C

import numpy as np


def n_tiles(n_rays, spr):
    return (n_rays * spr + 127) // 128


def table(native, n_rays, spr, enabled):
    """first sample slot of (workgroup tile, wave) in launch order -> int32 (n_tiles, 4)"""
    out = np.full(4 * n_tiles(n_rays, spr), -1, np.int32)
    rc = native.load_library().nerf_debug_ray_grouping(n_rays, spr, int(enabled), out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return out.reshape(-1, 4)


def grouped(n_rays, spr, enabled=True):
    """The issue's three conditions."""
    return bool(enabled) and spr % 32 == 0 and n_rays >= 4


# Case f of zero_skip_cases.py ("half-space empty": sigma exactly 0 on x < 0 and up to x = 0.04, positive beyond) as coarse and fine
# network, under the 800 x 800 lego camera, which looks down -y from x = -0.054 with +x on its left.  One row of 16 rays that ends 4 columns
# right of the centre: the 8 on the left start in x < 0 -- their first 32 fine samples see no density, the other five segments do -- and
# the 8 on the right never leave the empty half-space.  Ungrouped, a workgroup tile holds samples 0..127 or 128..191 + 0..63 or 64..191 of
# the left rays and is never empty there; grouped, the tile with segment 0 of four left rays is.  64 + 128 samples, seed 0.
F_ROW_WINDOW = (388, 405, 16, 1)
# A sample counts as a certain zero if the oracle's density PRE-activation is below -PRE_MARGIN (read from a twin network whose alpha
# bias is that much higher: its sigma is still 0), and as certainly positive if the oracle's sigma is above SIGMA_CERTAIN.  The device's
# density is held to 1e-4 (1 + sigma) of the oracle's everywhere in this suite, and its sample positions to a few ulp (1e-6 in x, 3e-5 in this
# network's pre-activation): both thresholds are a hundred times that or more.
PRE_MARGIN = 0.01
SIGMA_CERTAIN = 1e-2


def case_f_fine_samples(oracle, samples, net_dir, twin_dir, window=F_ROW_WINDOW, n_coarse=64, n_fine=128, seed=0):
    """The fine pass of that render, ray by ray from the oracle -> (zero, positive): (n_rays * (n_coarse + n_fine),) bool in sample order.
    twin_dir: where the twin network is written."""
    import zero_skip_cases as Z
    x0, y0, w, h = window
    cam = oracle.camera_from_samples(samples, 800, 800)
    net = oracle.Net(net_dir)
    Z._copy_net(net_dir, str(twin_dir))
    Z._edit(str(twin_dir), "alpha_bias", lambda b: b.__setitem__(slice(None), b + np.float32(PRE_MARGIN)))
    twin = oracle.Net(str(twin_dir))
    opts = oracle.make_opts(n_coarse, n_fine, seed=seed)
    o = np.float32(samples["camera_origin"])
    zero, positive = [], []
    for i in range(y0, y0 + h):
        for j in range(x0, x0 + w):
            ray = oracle.render_ray_debug(net, net, cam, opts, i, j)
            d, t = ray["dir_hat"], ray["t_merged"]
            p = (o[:, None] + (d[:, None] * t[None, :]).astype(np.float32)).astype(np.float32)      # src/lib.rs:436, rounded product then sum
            lifted = twin.forward_batch(np.ascontiguousarray(p), np.tile(d, (t.size, 1)))[1]
            zero.append((lifted == 0) & (ray["sigma_fine"] == 0))
            positive.append(ray["sigma_fine"] > SIGMA_CERTAIN)
    return np.concatenate(zero), np.concatenate(positive)


def empty_tiles(tab, zero, positive):
    """Workgroup tiles that skip_empty skips under mapping `tab`: those none of whose valid points (slot < n) has sigma > 0.  `zero` /
    `positive` (n,) bool: sigma certainly == 0 / certainly > 0 on the device.  -> (certainly skipped, possibly skipped) tile counts; the two
    are equal iff no tile's fate hangs on a point that is neither."""
    n = zero.size
    lo = hi = 0
    for waves in tab:
        idx = np.concatenate([np.arange(s, min(s + 32, n)) for s in waves if s < n]).astype(np.int64)
        lo += bool(zero[idx].all())
        hi += not positive[idx].any()
    return lo, hi
