"""Ray grouping of the f32 ray-mode MLP kernels (mlp_layout.h ray_group_first_slot), asked through nerf_debug_ray_grouping -- the function
the kernel calls, on the host.  The four waves of a workgroup tile take the same 32-sample segment of four neighbouring rays instead of 128
consecutive samples; the mapping must be a permutation of the launch's wave tiles, and the identity wherever grouping is off."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_grouping_cases as G  # noqa: E402

N_RAYS = (1, 3, 4, 5, 7, 8, 273, 384)
SPR = (32, 64, 128, 192, 70, 20)


def _identity(n_rays, spr):
    return (32 * np.arange(4 * G.n_tiles(n_rays, spr), dtype=np.int32)).reshape(-1, 4)


@pytest.mark.parametrize("enabled", (1, 0))
@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_wave_tiles_are_a_permutation(native, n_rays, spr, enabled):
    """Every first slot 0, 32, ... of the launch's 4 x n_tiles wave tiles exactly once: nothing missing, nothing doubled -- the tail past the
    last multiple of 32 (a partly valid wave) and the wholly invalid waves of the last workgroup tile included, as today."""
    tab = G.table(native, n_rays, spr, enabled)
    assert tab.shape == (G.n_tiles(n_rays, spr), 4)
    assert np.array_equal(np.sort(tab.reshape(-1)), _identity(n_rays, spr).reshape(-1))
    n = n_rays * spr
    assert (tab.reshape(-1) < n).sum() == (n + 31) // 32                       # the waves that hold a valid point cover [0, n)


@pytest.mark.parametrize("enabled", (1, 0))
@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("n_rays", N_RAYS)
def test_identity_where_grouping_is_off(native, n_rays, spr, enabled):
    """Switched off, samples per ray no multiple of 32, fewer than four rays, or one segment per ray (S = 1): 128 consecutive samples."""
    tab = G.table(native, n_rays, spr, enabled)
    if not G.grouped(n_rays, spr, enabled) or spr == 32:
        assert np.array_equal(tab, _identity(n_rays, spr))
    else:
        assert not np.array_equal(tab, _identity(n_rays, spr))                 # ... and it IS another mapping everywhere else


@pytest.mark.parametrize("spr", [s for s in SPR if s % 32 == 0])
@pytest.mark.parametrize("n_rays", [n for n in N_RAYS if n >= 4])
def test_grouped_tile_holds_one_segment_of_four_rays(native, n_rays, spr):
    """Wave w of workgroup tile T = b S + j holds segment j of ray 4 b + w, for every b < n_rays / 4, j < S, w < 4; the last n_rays % 4
    rays keep the identity."""
    tab = G.table(native, n_rays, spr, 1)
    S = spr // 32
    group_tiles = (n_rays // 4) * S
    for b in range(n_rays // 4):
        for j in range(S):
            for w in range(4):
                assert tab[b * S + j, w] == (4 * b + w) * spr + 32 * j, (b, j, w)
    assert np.array_equal(tab[group_tiles:], _identity(n_rays, spr)[group_tiles:])
    rest = tab[group_tiles:].reshape(-1)
    first_rest = (n_rays - n_rays % 4) * spr
    assert np.array_equal(rest[rest < n_rays * spr], np.arange(first_rest, n_rays * spr, 32))   # exactly the slots of those rays


def test_half_space_window_tells_the_mappings_apart(native, oracle, samples, tmp_path):
    """The window of test_gpu_ray_grouping.py's device check: with the half-space-empty network, the number of workgroup tiles without
    density is certain under both mappings (no tile's fate hangs on a sample near x = 0) and is not the same number."""
    from fold_utils import write_random_net
    import zero_skip_cases as Z
    d = Z._make_case("f", write_random_net(tmp_path / "net", 20240), tmp_path, oracle)[0]
    zero, positive = G.case_f_fine_samples(oracle, samples, d, tmp_path / "f_lifted")
    x0, y0, w, h = G.F_ROW_WINDOW
    n_rays, spr = w * h, 192
    assert zero.size == n_rays * spr and not (zero & positive).any()
    seg_zero, seg_pos = zero.reshape(n_rays, 6, 32).all(axis=2), positive.reshape(n_rays, 6, 32).any(axis=2)
    assert seg_zero[:8, 0].all() and seg_pos[:8, 1:].all()                     # the left rays: an empty depth range, then density
    assert seg_zero[8:].all()                                                  # the right rays: nothing
    want = {}
    for enabled in (0, 1):
        lo, hi = G.empty_tiles(G.table(native, n_rays, spr, enabled), zero, positive)
        print(f"\n{G.F_ROW_WINDOW} grouping {enabled}: {lo} .. {hi} of {G.n_tiles(n_rays, spr)} workgroup tiles are empty")
        assert lo == hi
        want[enabled] = lo
    assert 0 < want[0] < want[1] < G.n_tiles(n_rays, spr)


def test_rejects_bad_arguments(native):
    L = native.load_library()
    out = (C.c_int32 * 8)()
    assert L.nerf_debug_ray_grouping(0, 64, 1, out) != 0
    assert L.nerf_debug_ray_grouping(4, 0, 1, out) != 0
    assert L.nerf_debug_ray_grouping(4, 64, 1, None) != 0
    assert L.nerf_debug_ray_grouping(1 << 24, 192, 1, out) != 0               # more samples than one launch indexes
