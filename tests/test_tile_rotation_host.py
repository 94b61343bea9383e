"""Tile rotation of the fused f32 kernel (mlp_layout.h rotated_tile / tile_walk_next) on the host: nerf_debug_tile_rotation runs the kernel's
own walk for every persistent workgroup.  Round k's tile of workgroup c of G is k G + ((c + k) mod G); over all c and k that must enumerate
every tile below n_tiles exactly once, for any G and n_tiles -- a tile lost or taken twice would lose or double 128 points silently."""
import ctypes as C

import numpy as np
import pytest

I32P = C.POINTER(C.c_int32)


def _walk(native, n_tiles, G, rotation):
    who, rnd = np.full(n_tiles, -9, np.int32), np.full(n_tiles, -9, np.int32)
    rc = native.load_library().nerf_debug_tile_rotation(n_tiles, G, int(rotation), who.ctypes.data_as(I32P), rnd.ctypes.data_as(I32P))
    assert rc == 0, rc
    return who, rnd


@pytest.mark.parametrize("G", (1, 3, 256))
def test_every_tile_exactly_once(native, G):
    for n_tiles in sorted({1, max(G - 1, 1), G, G + 1, 5 * G + 7}):
        for rotation in (True, False):
            who, rnd = _walk(native, n_tiles, G, rotation)
            what = (G, n_tiles, rotation)
            assert (who >= 0).all() and (who < G).all(), what            # -1: nobody's, -2: taken twice
            t = np.arange(n_tiles)
            assert np.array_equal(rnd, t // G), what                     # round k holds tiles k G .. k G + G - 1
            want = (t % G - rnd) % G if rotation else t % G              # tile k G + r is workgroup c with (c + k) mod G = r
            assert np.array_equal(who, want), what
            for k in range(rnd.max() + 1):                               # a round is a permutation of its workgroups
                assert len(set(who[rnd == k])) == int((rnd == k).sum()), what


def test_a_workgroup_walks_through_all_positions(native):
    """What the rotation is for: with G = 256 and a period of 64 tiles, workgroup c of an unrotated launch only ever sees position c mod 64;
    rotated, 64 consecutive rounds show it all 64."""
    who, rnd = _walk(native, 64 * 256, 256, True)
    pos = np.arange(64 * 256) % 64
    assert {len(set(pos[who == c])) for c in range(256)} == {64}
    who, _ = _walk(native, 64 * 256, 256, False)
    assert {len(set(pos[who == c])) for c in range(256)} == {1}


def test_argument_errors(native):
    L = native.load_library()
    out = np.zeros(8, np.int32).ctypes.data_as(I32P)
    assert L.nerf_debug_tile_rotation(0, 4, 1, out, out) != 0
    assert L.nerf_debug_tile_rotation(4, 0, 1, out, out) != 0
    assert L.nerf_debug_tile_rotation(4, 4, 1, None, out) != 0
    assert L.nerf_debug_tile_rotation(4, 4, 1, out, None) != 0
    assert L.nerf_debug_tile_rotation(2 ** 31 - 10, 256, 1, out, out) != 0
