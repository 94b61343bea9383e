"""The unit walk of the coarse cut (mlp_layout.h RayCutWalk: ray_cut_walk_of / ray_cut_unit_tile / ray_cut_next_in_unit) on the host:
nerf_debug_coarse_cut_walk runs the functions the kernel's workgroups call, unit after unit.  With no block cut the walk visits every workgroup
tile of the launch exactly once; with block b cut behind its tile k it leaves out exactly the tiles of b behind k.  A block's tiles are
spr / 4 consecutive tiles of the ungrouped wave-tiling table (nerf_debug_wave_tiling), in which wave w of the block's tile k holds sample index
4 k + w of the block's 32 rays -- what lets a lane keep its ray for the whole block.  No device needed."""
import ctypes as C

import numpy as np
import pytest

I32P = C.POINTER(C.c_int32)
# (rows, rays per row): one block; 3 x 3 and 5 x 5 blocks; the bench frame; 20 = 5 x 4 rows; 22 rows leave two rows behind the blocks, and a row
# of 44 rays is no multiple of 8 (the sampling launch then has no 8 x 4 x 1 tiling and does not qualify)
SHAPES = [(4, 8), (12, 24), (20, 40), (800, 800), (22, 40), (20, 44), (3, 8)]
SPR = (4, 8, 64)


def _walk(native, rows, rw, spr, grouping=1, cut_block=-1, cut_after=0):
    n_tiles = (rows * rw * spr + 127) // 128
    tiles = np.full(n_tiles, -1, np.int32)
    blocks, block_tiles = C.c_int32(-1), C.c_int32(-1)
    n = native.load_library().nerf_debug_coarse_cut_walk(rows, rw, spr, grouping, cut_block, cut_after, tiles.ctypes.data_as(I32P), tiles.size,
                                                         C.byref(blocks), C.byref(block_tiles))
    assert n >= 0, n
    return tiles[:n], blocks.value, block_tiles.value, n_tiles


def _qualifies(rows, rw, spr):
    return spr % 32 == 0 and rows >= 4 and rw % 8 == 0


@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_uncut_walk_visits_every_tile_once(native, rows, rw, spr):
    tiles, blocks, block_tiles, n_tiles = _walk(native, rows, rw, spr)
    assert np.array_equal(np.sort(tiles), np.arange(n_tiles)), (rows, rw, spr)
    if _qualifies(rows, rw, spr):
        assert blocks == (rows // 4) * (rw // 8) and block_tiles == spr // 4
    else:
        assert blocks == 0                                                    # the launch keeps its static walk
    for grouping in (0, 1):                                                    # the tiled region is ungrouped either way
        again, b2, _, _ = _walk(native, rows, rw, spr, grouping)
        assert np.array_equal(again, tiles) and b2 == blocks


@pytest.mark.parametrize("rows,rw", [(12, 24), (22, 40), (800, 800)])
def test_cut_walk_leaves_out_the_tiles_behind_the_cut(native, rows, rw):
    spr = 64
    full, blocks, block_tiles, n_tiles = _walk(native, rows, rw, spr)
    assert block_tiles == 16 and blocks > 1
    for b in sorted({0, 1, blocks // 2, blocks - 1}):
        for k in (0, 1, 7, block_tiles - 2, block_tiles - 1):
            tiles, _, _, _ = _walk(native, rows, rw, spr, 1, b, k)
            gone = np.arange(b * block_tiles + k + 1, (b + 1) * block_tiles)
            assert len(tiles) == n_tiles - len(gone), (b, k)
            assert np.array_equal(np.sort(tiles), np.setdiff1d(np.arange(n_tiles), gone)), (b, k)
            assert np.array_equal(tiles, full[~np.isin(full, gone)]), (b, k)   # the other tiles keep their order
    # block_tiles = 1 (spr = 4 never qualifies: the tiling needs a multiple of 32); a cut behind a block's last tile removes nothing
    tiles, _, _, _ = _walk(native, rows, rw, spr, 1, 0, block_tiles - 1)
    assert np.array_equal(tiles, full)


@pytest.mark.parametrize("rows,rw,spr", [(4, 8, 32), (12, 24, 64), (22, 40, 64), (9, 16, 96)])
def test_a_block_is_consecutive_tiles_of_one_pixel_block_front_to_back(native, rows, rw, spr):
    """The table of the ungrouped tiled map: lane p of wave w of tile k of block b holds sample 4 k + w of ray (4 by + p / 8, 8 bx + p % 8)."""
    tiles, blocks, block_tiles, n_tiles = _walk(native, rows, rw, spr)
    slot = np.empty(n_tiles * 128, np.int32)
    assert native.load_library().nerf_debug_wave_tiling(rows, rw, spr, 0, 0, 1, slot.ctypes.data_as(I32P)) == 0
    slot = slot.reshape(n_tiles, 4, 32)
    assert blocks == (rows // 4) * (rw // 8)
    assert np.array_equal(tiles[:blocks * block_tiles], np.arange(blocks * block_tiles))   # block after block, each front to back
    p = np.arange(32)
    for b in range(blocks):
        by, bx = divmod(b, rw // 8)
        ray = (4 * by + p // 8) * rw + 8 * bx + p % 8
        for k in range(block_tiles):
            for w in range(4):
                assert np.array_equal(slot[b * block_tiles + k, w], ray * spr + 4 * k + w), (b, k, w)
    rest = slot[blocks * block_tiles:].reshape(-1)                              # the rows behind the blocks: every other slot once
    rest = rest[rest >= 0]
    assert np.array_equal(np.sort(rest), np.arange(blocks * 32 * spr, rows * rw * spr))


def test_refusals(native):
    L = native.load_library()
    out = (C.c_int32 * 8)()
    assert L.nerf_debug_coarse_cut_walk(0, 8, 64, 1, -1, 0, out, 8, None, None) < 0
    assert L.nerf_debug_coarse_cut_walk(4, 8, 64, 1, -1, 0, None, 8, None, None) < 0
    assert L.nerf_debug_coarse_cut_walk(4, 8, 64, 1, -1, 0, out, 8, None, None) < 0      # 16 tiles do not fit 8 entries
    assert L.nerf_debug_coarse_cut_walk(2 ** 15, 2 ** 15, 64, 1, -1, 0, out, 8, None, None) < 0
