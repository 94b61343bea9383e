"""The unit walk of the fine cut (mlp_layout.h fine_cut_walk_of / ray_cut_unit_tile / ray_cut_next_in_unit) on the host:
nerf_debug_fine_cut_walk runs the functions the kernel's workgroups call, unit after unit.  A unit is a pixel block of the depth-ordered
region -- the spr / 4 consecutive tiles of its part of the order table -- or one tile of the rows behind it.  With no block cut the walk visits
every workgroup tile of the launch exactly once; with block b cut behind its tile k it leaves out exactly the tiles of b behind k.  No device
needed."""
import ctypes as C

import numpy as np
import pytest

I32P = C.POINTER(C.c_int32)
# (rows, rays per row): one block (fewer blocks than any device has workgroups); nine blocks; 25 blocks, whole blocks only; the bench frame; 22
# and 10 rows leave two tail rows behind the blocks; a row of 44 rays is no multiple of 8 and three rows are fewer than a block's four: such a
# launch is not depth-ordered and does not qualify
SHAPES = [(4, 8), (12, 24), (20, 40), (800, 800), (22, 40), (10, 32), (20, 44), (3, 8)]
SPR = (8, 64, 96, 192)


def _walk(native, rows, rw, spr, cut_block=-1, cut_after=0):
    n_tiles = (rows * rw * spr + 127) // 128
    tiles = np.full(n_tiles, -1, np.int32)
    blocks, block_tiles = C.c_int32(-1), C.c_int32(-1)
    n = native.load_library().nerf_debug_fine_cut_walk(rows, rw, spr, cut_block, cut_after, tiles.ctypes.data_as(I32P), tiles.size,
                                                       C.byref(blocks), C.byref(block_tiles))
    assert n >= 0, n
    return tiles[:n], blocks.value, block_tiles.value, n_tiles


def _qualifies(rows, rw, spr):
    return spr % 32 == 0 and spr <= 512 and rows >= 4 and rw % 8 == 0


@pytest.mark.parametrize("spr", SPR)
@pytest.mark.parametrize("rows,rw", SHAPES)
def test_uncut_walk_visits_every_tile_once(native, rows, rw, spr):
    tiles, blocks, block_tiles, n_tiles = _walk(native, rows, rw, spr)
    assert np.array_equal(np.sort(tiles), np.arange(n_tiles)), (rows, rw, spr)
    if _qualifies(rows, rw, spr):
        assert blocks == (rows // 4) * (rw // 8) and block_tiles == spr // 4
        assert np.array_equal(tiles[:blocks * block_tiles], np.arange(blocks * block_tiles))   # block after block, each front to back
        assert blocks * block_tiles * 128 == (rows // 4) * 4 * rw * spr                        # the ordered region, whole tiles
    else:
        assert blocks == 0                                                                     # the launch keeps its static walk


@pytest.mark.parametrize("rows,rw", [(4, 8), (12, 24), (22, 40), (10, 32), (800, 800)])
def test_cut_walk_leaves_out_the_tiles_behind_the_cut(native, rows, rw):
    spr = 192
    full, blocks, block_tiles, n_tiles = _walk(native, rows, rw, spr)
    assert block_tiles == 48 and blocks >= 1
    for b in sorted({0, 1 % blocks, blocks // 2, blocks - 1}):
        for k in (0, 1, 17, block_tiles - 2, block_tiles - 1):
            tiles, _, _, _ = _walk(native, rows, rw, spr, b, k)
            gone = np.arange(b * block_tiles + k + 1, (b + 1) * block_tiles)
            assert len(tiles) == n_tiles - len(gone), (b, k)
            assert np.array_equal(np.sort(tiles), np.setdiff1d(np.arange(n_tiles), gone)), (b, k)
            assert np.array_equal(tiles, full[~np.isin(full, gone)]), (b, k)                   # the other tiles keep their order
    tiles, _, _, _ = _walk(native, rows, rw, spr, 0, block_tiles - 1)                          # a cut behind a block's last tile removes nothing
    assert np.array_equal(tiles, full)
    tiles, _, _, _ = _walk(native, rows, rw, spr, blocks, 0)                                   # a tile behind the blocks is never "cut"
    assert np.array_equal(tiles, full)


def test_refusals(native):
    L = native.load_library()
    out = (C.c_int32 * 8)()
    assert L.nerf_debug_fine_cut_walk(0, 8, 64, -1, 0, out, 8, None, None) < 0
    assert L.nerf_debug_fine_cut_walk(4, 8, 64, -1, 0, None, 8, None, None) < 0
    assert L.nerf_debug_fine_cut_walk(4, 8, 64, -1, 0, out, 8, None, None) < 0      # 16 tiles do not fit 8 entries
    assert L.nerf_debug_fine_cut_walk(2 ** 15, 2 ** 15, 64, -1, 0, out, 8, None, None) < 0
