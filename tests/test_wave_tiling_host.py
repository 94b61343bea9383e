"""Wave tiling of the f32 ray-mode MLP kernels (mlp_layout.h ray_launch_slot), asked lane by lane through nerf_debug_wave_tiling -- the
functions the kernel calls, on the host.  In an image pass a wave holds ss consecutive samples of each ray of a tw x th block of pixels
instead of 32 consecutive samples of one ray; the mapping must be a permutation of the launch's points, nerf_debug_ray_grouping's table
wherever a launch is not tiled, and block-shaped where it is."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ray_grouping_cases as G  # noqa: E402
import wave_tiling_cases as W  # noqa: E402

SHAPES = ((4, 8), (4, 32), (8, 32), (5, 33), (13, 21), (16, 24), (2, 4), (3, 4), (1, 16), (6, 12), (2, 42))   # (rows, rays per row)
SPR = (32, 64, 128, 192, 70)
KINDS = [(full, grouping, tiling) for full in (False, True) for grouping in (True, False) for tiling in (True, False)]


def _tiled_tiles(rows, rw, spr, shape):
    return 0 if shape is None else (rows // shape[1]) * shape[1] * rw * spr // 128


@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_every_point_exactly_once(native, rows, rw, spr):
    """A permutation of [0, n_points); padding lanes (-1) in the launch's last workgroup tile only."""
    n = rows * rw * spr
    for full, grouping, tiling in KINDS:
        tab = W.table(native, rows, rw, spr, full, grouping, tiling)
        assert tab.shape == (W.n_tiles(rows, rw, spr), 4, 32)
        flat = tab.reshape(-1)
        assert np.array_equal(np.sort(flat[flat >= 0]), np.arange(n)), (full, grouping, tiling)
        assert (flat >= -1).all() and (tab[:-1] >= 0).all(), (full, grouping, tiling)
        assert (flat < 0).sum() == 128 * W.n_tiles(rows, rw, spr) - n


@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_untiled_launches_keep_the_ray_grouping_table(native, rows, rw, spr):
    """Switched off, samples per ray no multiple of 32, fewer rows than the block is high, or no block of 4 pixels whose width divides the
    row: first slot of nerf_debug_ray_grouping + lane.  Everywhere else it is another mapping."""
    for full, grouping, tiling in KINDS:
        tab = W.table(native, rows, rw, spr, full, grouping, tiling)
        same = np.array_equal(tab, W.untiled_table(native, rows * rw, spr, grouping))
        assert same == (W.shape_of(rows, rw, spr, full, tiling) is None), (full, grouping, tiling)


def test_the_rules_name_the_expected_launches():
    """The restated rules against the cases the design names: 70 samples, one row, 21 rays per row for the full kind, rows < th."""
    assert W.shape_of(8, 32, 70, False) is None and W.shape_of(8, 32, 70, True) is None
    assert W.shape_of(1, 16, 64, False) is None and W.shape_of(1, 16, 64, True) is None
    assert W.shape_of(13, 21, 64, True) is None and W.shape_of(13, 21, 64, False) == (1, 4, 8)
    assert W.shape_of(3, 4, 64, False) is None and W.shape_of(3, 4, 64, True) == (4, 2, 4)
    assert W.shape_of(2, 4, 192, False) is None and W.shape_of(2, 42, 192, False) is None
    assert W.shape_of(8, 32, 64, False) == (8, 4, 1) and W.shape_of(8, 32, 192, True) == (4, 2, 4)
    assert W.shape_of(2, 42, 192, True) == (2, 2, 8) and W.shape_of(4, 42, 64, False) == (2, 4, 4)
    assert W.shape_of(8, 32, 64, False, tiling=False) is None


@pytest.mark.parametrize("spr", [s for s in SPR if s % 32 == 0])
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_tiled_waves_are_pixel_blocks(native, rows, rw, spr):
    """In the tiled region a wave holds exactly the tw x th pixels of one bundle x ss consecutive samples of one aligned segment, in lane
    order (dy, dx, ds); grouped, the four waves of a workgroup tile hold the same segment of four consecutive bundles, ungrouped (and for the
    last n_bundles % 4 bundles) four consecutive segments of one bundle."""
    for full in (False, True):
        shape = W.shape_of(rows, rw, spr, full)
        if shape is None:
            continue
        tw, th, ss = shape
        S_t, bx_n = spr // ss, rw // tw
        n_bundles = bx_n * (rows // th)
        nt = _tiled_tiles(rows, rw, spr, shape)
        assert nt * 4 == n_bundles * S_t and S_t % 4 == 0
        p = np.arange(32)
        ds, dx, dy = p % ss, (p // ss) % tw, p // (ss * tw)
        for grouping in (True, False):
            tab = W.table(native, rows, rw, spr, full, grouping, True)[:nt].astype(np.int64)
            ray, smp = tab // spr, tab % spr
            py, px = ray // rw, ray % rw
            by, bx, j = py[:, :, 0] // th, px[:, :, 0] // tw, smp[:, :, 0] // ss
            assert np.array_equal(py, (by * th)[:, :, None] + dy) and np.array_equal(px, (bx * tw)[:, :, None] + dx)
            assert np.array_equal(smp, (j * ss)[:, :, None] + ds)
            assert (by < rows // th).all() and (j < S_t).all()
            for wave in tab.reshape(-1, 32):                       # ... which makes every wave tw th distinct pixels x ss distinct samples
                assert len(set(wave // spr)) == tw * th and len(set(wave % spr)) == ss
            bundle = by * bx_n + bx
            grouped = (n_bundles // 4) * S_t if grouping and n_bundles >= 4 else 0
            T = np.arange(grouped)
            for w in range(4):
                assert np.array_equal(bundle[:grouped, w], 4 * (T // S_t) + w) and np.array_equal(j[:grouped, w], T % S_t)
            wave_tile = (bundle * S_t + j)[grouped:]
            assert np.array_equal(wave_tile.reshape(-1), 4 * grouped + np.arange(4 * (nt - grouped)))


@pytest.mark.parametrize("spr", [s for s in SPR if s % 32 == 0])
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_tail_rows_map_as_an_untiled_launch_of_those_rows(native, rows, rw, spr):
    """The last rows % th rows: contiguous slots behind the tiled region, mapped like an untiled launch of just those rows, shifted."""
    for full, grouping in ((False, True), (False, False), (True, True), (True, False)):
        shape = W.shape_of(rows, rw, spr, full)
        if shape is None:
            continue
        nt, tail_rows = _tiled_tiles(rows, rw, spr, shape), rows % shape[1]
        tab = W.table(native, rows, rw, spr, full, grouping, True)
        assert tab[:nt].max() == nt * 128 - 1
        if tail_rows == 0:
            assert tab.shape[0] == nt
        else:
            assert np.array_equal(tab[nt:], W.untiled_table(native, tail_rows * rw, spr, grouping, shift=128 * nt))


def test_half_space_window_tells_tiled_from_untiled(native, oracle, samples, tmp_path):
    """The window of test_gpu_wave_tiling.py's device check: with the half-space-empty network the number of workgroup tiles without density
    is certain under the default mapping and under the untiled one (no tile's fate hangs on a sample near x = 0), and not the same number."""
    from fold_utils import write_random_net
    import zero_skip_cases as Z
    d = Z._make_case("f", write_random_net(tmp_path / "net", 20240), tmp_path, oracle)[0]
    x0, y0, w, h = W.F_BLOCK_WINDOW
    zero, positive = G.case_f_fine_samples(oracle, samples, d, tmp_path / "f_lifted", window=W.F_BLOCK_WINDOW)
    assert zero.size == w * h * 192 and not (zero & positive).any()
    assert W.shape_of(h, w, 192, True) == (4, 2, 4)
    want = {}
    for tiling in (False, True):
        lo, hi = W.empty_tiles(W.table(native, h, w, 192, True, True, tiling), zero, positive)
        print(f"\n{W.F_BLOCK_WINDOW} tiling {tiling}: {lo} .. {hi} of {W.n_tiles(h, w, 192)} workgroup tiles are empty")
        assert lo == hi
        want[tiling] = lo
    assert 0 < want[True] < want[False] < W.n_tiles(h, w, 192)
    # the per-lane count is the per-wave-tile one of ray_grouping_cases where the table is that one
    assert W.empty_tiles(W.table(native, h, w, 192, True, True, False), zero, positive) == G.empty_tiles(G.table(native, w * h, 192, 1), zero, positive)


def test_rejects_bad_arguments(native):
    L = native.load_library()
    out = (C.c_int32 * 128)()
    assert L.nerf_debug_wave_tiling(0, 4, 64, 0, 1, 1, out) != 0
    assert L.nerf_debug_wave_tiling(1, 0, 64, 0, 1, 1, out) != 0
    assert L.nerf_debug_wave_tiling(1, 4, 0, 0, 1, 1, out) != 0
    assert L.nerf_debug_wave_tiling(1, 2, 32, 0, 1, 1, None) != 0
    assert L.nerf_debug_wave_tiling(1 << 12, 1 << 12, 192, 1, 1, 1, out) != 0       # more samples than one launch indexes
