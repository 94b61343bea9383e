"""What the wave-tiling tests share (test_wave_tiling_host.py, test_gpu_wave_tiling.py): the lane-by-lane mapping table as the library
reports it (nerf_debug_wave_tiling calls the functions the f32 ray-mode kernels call, mlp_layout.h ray_launch_slot), the rules for when a
launch is tiled restated from the design, and what skip_empty and the zero-step counters must give under a table.  Nothing here
needs a GPU."""
import ctypes as C

import numpy as np

# pixel block a pass kind starts from: (tw, th); the sigma-only sampling launch / the launch that produces colours
START = {False: (8, 4), True: (4, 2)}


def n_tiles(rows, rw, spr):
    return (rows * rw * spr + 127) // 128


def table(native, rows, rw, spr, full, grouping, tiling):
    """sample slot of (workgroup tile, wave, lane) in launch order, -1 = padding lane -> int32 (n_tiles, 4, 32)"""
    out = np.full(128 * n_tiles(rows, rw, spr), -7, np.int32)
    rc = native.load_library().nerf_debug_wave_tiling(rows, rw, spr, int(full), int(grouping), int(tiling), out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return out.reshape(-1, 4, 32)


def shape_of(rows, rw, spr, full, tiling=True):
    """(tw, th, ss) of a tiled launch, None where the rules say untiled: switched off, samples per ray no multiple of 32, fewer rows than the
    block is high, or -- after halving tw until it divides rw -- a block of fewer than 4 pixels."""
    tw, th = START[bool(full)]
    if not tiling or spr % 32 != 0:
        return None
    while rw % tw:
        tw //= 2
    if rows < th or tw * th < 4:
        return None
    return tw, th, 32 // (tw * th)


def untiled_table(native, n_rays, spr, grouping, shift=0):
    """nerf_debug_ray_grouping's table spelled out lane by lane (first slot + lane; -1 beyond the launch), slots shifted by `shift`"""
    import ray_grouping_cases as G
    first = G.table(native, n_rays, spr, grouping).astype(np.int64)
    s = first[:, :, None] + np.arange(32)
    return np.where(s < n_rays * spr, s + shift, -1).astype(np.int32)


def empty_tiles(tab, zero, positive):
    """ray_grouping_cases.empty_tiles for a lane-by-lane table: workgroup tiles none of whose valid lanes has sigma > 0 -> (certainly
    skipped, possibly skipped) tile counts; equal iff no tile's fate hangs on a sample that is neither a certain zero nor certainly positive."""
    lo = hi = 0
    for lanes in tab.reshape(tab.shape[0], -1):
        idx = lanes[lanes >= 0].astype(np.int64)
        lo += bool(zero[idx].all())
        hi += not positive[idx].any()
    return lo, hi


def kstep_bracket(tab, pre_list, eps):
    """zero_skip_cases.kstep_bracket over the waves of a lane-by-lane table: pre_list = float64 pre-activations (n_points, 256) per ReLU-input
    layer in SLOT order; a padding lane repeats the launch's last point, as the kernels' clamped loads do -> (certain_live, certain_dead, total)"""
    import zero_skip_cases as Z
    n = pre_list[0].shape[0]
    idx = np.where(tab >= 0, tab, n - 1).reshape(-1, 32).astype(np.int64)      # (waves, 32)
    live = dead = total = 0
    for z in pre_list:
        w = z[idx][:, :, Z.STEP_UNITS]                                          # (waves, 32 points, 128 steps, 2 units)
        hi = w.max(axis=(1, 3))
        assert not np.isnan(hi).any()
        live += int((hi > eps).sum()); dead += int((hi < -eps).sum()); total += hi.size
    return live, dead, total


# Case f of zero_skip_cases.py (the half-space-empty network) under ray_grouping_cases.F_ROW_WINDOW's geometry, two rows high: 16 x 2 rays,
# the 8 columns on the left cross from an empty first 32 fine samples into density, the 8 on the right see nothing.  The full launch tiles it
# in four 4 x 2 bundles x 4 samples: by default the four waves of workgroup tile j hold samples 4 j .. 4 j + 3 of all four bundles, so a tile is
# empty only while the left bundles are (j < 8 of 48); untiled (grouped), the blocks of four right-hand rays are empty in all six segments and
# those of left-hand rays in the first.
F_BLOCK_WINDOW = (388, 405, 16, 2)
