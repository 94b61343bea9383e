"""CPU tests of the four 16-bit weight streams (host_util.cpp build_streams: every loader -- directory, tensors, blob -- builds them from
the packed f32 image), read through the host-only nerf_debug_network_stream_dir:
  * the streams of both lego networks against digests recorded from the two-path builders this function replaced (tests/golden);
  * a random network against a numpy restatement written from the layout comments of mlp_layout.h and the raw tensors alone;
  * a network with one weight beyond the f16 range: the two f16 streams are unavailable, the two bf16 streams unchanged in kind;
  * the size query and the short-buffer refusal."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENE
from fold_utils import raw_tensors, write_random_net

KINDS = {"bf16v2": 0, "f16v2": 1, "bf16x3": 2, "f16x2": 3}  # NERF_STREAM_* (include/nerf_mi355x.h)
u16p = C.POINTER(C.c_uint16)
PIECE = 512  # 16-bit elements of a 1-KiB piece: 64 lanes x 8


def stream(native, d, kind, expect_available=True):
    L = native.load_library()
    n, av = C.c_size_t(), C.c_int(-1)
    d = str(d).encode()
    assert L.nerf_debug_network_stream_dir(d, KINDS[kind], None, 0, C.byref(n), C.byref(av)) == 0
    assert av.value == int(expect_available)
    if not expect_available:
        assert n.value == 0
        return None
    a = np.empty(n.value, np.uint16)
    assert L.nerf_debug_network_stream_dir(d, KINDS[kind], a.ctypes.data_as(u16p), a.size, None, None) == 0
    return a


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_lego_streams_equal_the_recorded_digests(native, which):
    want = json.load(open(os.path.join(GOLDEN, "stream_digests.json")))[which]
    assert sorted(want) == sorted(KINDS)
    for kind in KINDS:
        a = stream(native, os.path.join(SCENE, which), kind)
        assert a.size == want[kind]["elements"], kind
        assert hashlib.sha256(a.tobytes()).hexdigest() == want[kind]["sha256"], kind


# ---- the restatement: mlp_layout.h in numpy, from the raw tensors -------------------------------------------------------------------
def reg_feature(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def pos_slot_feature(idx, h):
    if idx < 30:
        return 3 + 6 * (5 * h + idx // 6) + idx % 6
    return idx - 30 if h == 0 else (2 if idx == 30 else -1)


def dir_slot_feature(idx, h):
    if idx < 12:
        return 3 + 6 * (2 * h + idx // 6) + idx % 6
    return idx - 12 if (h == 0 and idx < 15) else -1


def hidden_row(tile, r, h):
    return 32 * tile + reg_feature(r, h)


def dense5_row(tile, r, h):      # rows 0..62 position encoding, 63..318 the skip connection's hidden units
    return pos_slot_feature(16 * tile + r, h) if tile < 2 else 63 + hidden_row(tile - 2, r, h)


def viewdirs_row(tile, r, h):    # rows 0..255 bottleneck, 256..282 direction encoding
    if tile < 8:
        return hidden_row(tile, r, h)
    f = dir_slot_feature(r, h)
    return -1 if f < 0 else 256 + f


LAYERS = [("dense0", 2, 8, lambda t, r, h: pos_slot_feature(16 * t + r, h))] + [(f"dense{i}", 8, 8, hidden_row) for i in range(1, 5)] + \
         [("dense5", 10, 8, dense5_row), ("dense6", 8, 8, hidden_row), ("dense7", 8, 8, hidden_row), ("bottleneck", 8, 8, hidden_row),
          ("viewdirs", 9, 4, viewdirs_row)]


def layer_pieces(W, in_tiles, NT, row):
    """[k-step (K = 16)][output tile][lane][element] float32: element j of lane l of piece (ks, nt) is
    W[row(ks >> 1, 8 (ks & 1) + j, l >> 5)][32 nt + (l & 31)], 0 where the slot is padding."""
    K, N = W.shape
    P = np.zeros((2 * in_tiles, NT, 64, 8), np.float32)
    for ks in range(2 * in_tiles):
        for h in (0, 1):
            for j in range(8):
                r = row(ks >> 1, 8 * (ks & 1) + j, h)
                if 0 <= r < K:
                    for nt in range(NT):
                        P[ks, nt, 32 * h:32 * h + 32, j] = W[r, 32 * nt:32 * nt + 32]
    return P


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_value(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split_bf16x3(v):
    p0 = bf16_rne(v); r1 = (v - bf16_value(p0)).astype(np.float32)
    p1 = bf16_rne(r1); r2 = (r1 - bf16_value(p1)).astype(np.float32)
    return np.stack([p0, p1, bf16_rne(r2)])


def split_f16x2(v):
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return np.stack([hi.view(np.uint16), lo.view(np.uint16)])


def restate(d):
    """kind -> uint16 stream of the weight directory d."""
    W = {k: v.astype(np.float32) for k, v in raw_tensors(d).items()}
    tile_major, step_major = [], []
    for name, in_tiles, NT, row in LAYERS:
        P = layer_pieces(W[name + "_kernel"], in_tiles, NT, row)
        tile_major.append(P.transpose(1, 0, 2, 3).reshape(-1))   # bf16v2 / f16v2: per output tile, per k-step
        step_major.append(P.reshape(-1, PIECE))                   # bf16x3 / f16x2: per k-step, per output tile; a unit = the piece's parts
    v2 = np.concatenate(tile_major + [np.zeros(8 * PIECE, np.float32)])  # viewdirs' 72 pieces padded to whole 16-piece chunks
    sm = np.concatenate(step_major)
    with np.errstate(over="ignore", invalid="ignore"):
        return {"bf16v2": bf16_rne(v2), "f16v2": v2.astype(np.float16).view(np.uint16),
                "bf16x3": np.stack([split_bf16x3(p) for p in sm]).reshape(-1), "f16x2": np.stack([split_f16x2(p) for p in sm]).reshape(-1)}


@pytest.fixture(scope="module")
def random_net(tmp_path_factory):
    return write_random_net(tmp_path_factory.mktemp("streams") / "net", 31337)


@pytest.fixture(scope="module")
def huge_weight_net(tmp_path_factory):
    d = write_random_net(tmp_path_factory.mktemp("streams_huge") / "net", 31337)
    p = os.path.join(d, "viewdirs_kernel.bin")
    w = np.fromfile(p, "<f4"); w[10 * 128 + 3] = 1e5; w.tofile(p)
    return d


def test_numpy_splits_are_the_debug_splitters(native, random_net):
    """the restatement's two splits, element for element, against nerf_debug_split_* (which define them) on a layer's weights and edge values"""
    L = native.load_library()
    v = np.concatenate([np.fromfile(os.path.join(random_net, "dense5_kernel.bin"), "<f4"),
                        np.float32([0.0, -0.0, 1.0, -3.14159274, 65504.0, 1e-8, 6e-8, 1e5, -1e30])])
    f32p = C.POINTER(C.c_float)
    p3, p2 = np.empty(3 * v.size, np.uint16), np.empty(2 * v.size, np.uint16)
    assert L.nerf_debug_split_bf16x3(v.ctypes.data_as(f32p), v.size, p3.ctypes.data_as(u16p)) == 0
    assert L.nerf_debug_split_f16x2(v.ctypes.data_as(f32p), v.size, p2.ctypes.data_as(u16p)) == 0
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.array_equal(split_bf16x3(v).T.reshape(-1), p3)
        fits = np.abs(v) <= 65504.0
        assert np.array_equal(split_f16x2(v).T[fits].reshape(-1), p2.reshape(-1, 2)[fits].reshape(-1))


def test_random_network_streams_equal_the_restatement(native, random_net):
    want = restate(random_net)
    for kind in KINDS:
        got = stream(native, random_net, kind)
        assert got.size == want[kind].size, kind
        assert np.array_equal(got, want[kind]), (kind, int((got != want[kind]).sum()))


def test_weight_beyond_f16_range_makes_the_f16_streams_unavailable(native, huge_weight_net):
    want = restate(huge_weight_net)
    for kind in ("f16x2", "f16v2"):
        assert stream(native, huge_weight_net, kind, expect_available=False) is None
    for kind in ("bf16v2", "bf16x3"):
        got = stream(native, huge_weight_net, kind)
        assert np.array_equal(got, want[kind]), kind
    assert np.uint16(0x47c3) in stream(native, huge_weight_net, "bf16v2")  # bf16(1e5) = 0x47c3 (99840): the weight is in the stream


def test_short_buffer_is_refused_and_nothing_is_written_past_cap(native, random_net):
    L = native.load_library()
    d = str(random_net).encode()
    for kind, k in KINDS.items():
        n = C.c_size_t()
        assert L.nerf_debug_network_stream_dir(d, k, None, 0, C.byref(n), None) == 0 and n.value > 0
        buf = np.full(n.value + 64, 0xA5A5, np.uint16)
        for cap in (0, 1, n.value - 1):
            rc = L.nerf_debug_network_stream_dir(d, k, buf.ctypes.data_as(u16p), cap, None, None)
            assert rc == -1 and b"stream buffer too small" in L.nerf_last_error(None), (kind, cap, rc)
            assert (buf == 0xA5A5).all(), (kind, cap)            # refused before anything is copied
        assert L.nerf_debug_network_stream_dir(d, k, buf.ctypes.data_as(u16p), n.value, None, None) == 0
        assert (buf[n.value:] == 0xA5A5).all() and (buf[:n.value] != 0xA5A5).any(), kind
    assert L.nerf_debug_network_stream_dir(d, 4, None, 0, C.byref(n), None) == -1
    assert L.nerf_debug_network_stream_dir(None, 0, None, 0, C.byref(n), None) == -1
