"""Helpers shared by test_fold_host.py (CPU) and test_gpu_fold.py: the folded image of the f32 kernels (mlp_layout.h
kChunksFullFolded: the activation-free bottleneck folded into the viewdirs layer), read through the host-only C ABI, its
un-permutation, the fp64 yardstick from the raw tensors, and networks of the reference's architecture with seeded weights."""
import ctypes as C
import os

import numpy as np

CHUNK = 4096                                     # floats per 16-KiB chunk
N_SIGMA, N_PACKED, N_FOLDED = 120, 145, 129      # chunks: dense0..7 | + bottleneck (16) + viewdirs (9) | + viewdirs' (8 + 1)
BIAS, BIASV = 0, 9 * 256                         # small block (floats): 9 x 256 layer biases, then the viewdirs bias [4 nt][2 h][16]
AW = BIASV + 128
RW = AW + 256
MISC = RW + 384
ROW_OF = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for h in (0, 1)] for r in range(16)])  # feature of register r on lane-half h
LANE = np.arange(64); P_ = LANE & 31; H_ = LANE >> 5

SHAPES = [("dense0", 63, 256)] + [(f"dense{i}", 256, 256) for i in range(1, 5)] + [("dense5", 319, 256), ("dense6", 256, 256),
          ("dense7", 256, 256), ("bottleneck", 256, 256), ("viewdirs", 283, 128), ("rgb", 128, 3), ("alpha", 256, 1)]


def image(native, d, folded):
    """(weight stream, small block) of a weight directory: the packed image, or the folded one the f32 kernels read."""
    L = native.load_library()
    fn = L.nerf_debug_fold_network_dir if folded else L.nerf_debug_pack_network_dir
    nw, ns = C.c_size_t(), C.c_size_t()
    d = str(d).encode()
    assert fn(d, None, 0, None, 0, C.byref(nw), C.byref(ns)) == 0
    ws = np.empty(nw.value, np.float32); sm = np.empty(ns.value, np.float32)
    f32p = C.POINTER(C.c_float)
    assert fn(d, ws.ctypes.data_as(f32p), ws.size, sm.ctypes.data_as(f32p), sm.size, None, None) == 0
    return ws, sm


def raw_tensors(d):
    """name -> float64 array, from shapes.txt + <name>.bin."""
    W = {}
    for line in open(os.path.join(str(d), "shapes.txt")):
        name, *dims = line.split()
        W[name] = np.fromfile(os.path.join(str(d), name + ".bin"), dtype="<f4").astype(np.float64).reshape([int(x) for x in dims])
    return W


def fold_fp64(d):
    """W' = W_b . W_v[0:256] and b' = b_v + b_b^T . W_v[0:256] in float64 from the raw tensors."""
    W = raw_tensors(d)
    wv = W["viewdirs_kernel"][:256]
    return W["bottleneck_kernel"] @ wv, W["viewdirs_bias"] + W["bottleneck_bias"] @ wv


def unpermute_folded(fws, fsm):
    """(W' [256][128], b' [128]) as float32 from the folded image: piece st of the 4-output-tile layer holds, for lane l and q,
    W'[32 (st >> 4) + ROW_OF[st & 15][l >> 5]][32 q + (l & 31)]."""
    pieces = fws[N_SIGMA * CHUNK: (N_SIGMA + 8) * CHUNK].reshape(128, 64, 4)
    Wf = np.full((256, 128), np.nan, np.float32)
    for st in range(128):
        rows = 32 * (st >> 4) + ROW_OF[st & 15][H_]
        for q in range(4):
            Wf[rows, 32 * q + P_] = pieces[st, :, q]
    bf = np.full(128, np.nan, np.float32)
    for nt in range(4):
        for h in (0, 1):
            bf[32 * nt + ROW_OF[:, h]] = fsm[BIASV + (nt * 2 + h) * 16: BIASV + (nt * 2 + h) * 16 + 16]
    assert not np.isnan(Wf).any() and not np.isnan(bf).any()          # every element was written: the layout is a permutation
    return Wf, bf


def write_random_net(d, seed, bottleneck_bias_scale=2.0, zero_bottleneck_kernel=False):
    """A network of the reference's architecture with seeded He-scaled weights in the reference's directory format.  The bottleneck
    bias is LARGE (N(0, 2^2) against N(0, 0.1^2) elsewhere): b_b^T W_v then dwarfs b_v, so a fold that loses or misplaces the bias
    term is far outside every tolerance.  zero_bottleneck_kernel: W_b = 0, so W' must be exactly 0 and the head sees b' alone."""
    rng = np.random.default_rng(seed)
    d = str(d)
    os.makedirs(d, exist_ok=True)
    lines = []
    for name, k, n in SHAPES:
        w = (rng.normal(size=(k, n)) * np.sqrt(2.0 / k)).astype("<f4")
        b = (rng.normal(size=(n,)) * 0.1).astype("<f4")
        if name == "alpha":
            b[:] = 0.7                                                   # keep a good share of the densities positive
        if name == "bottleneck":
            b = (rng.normal(size=(n,)) * bottleneck_bias_scale).astype("<f4")
            if zero_bottleneck_kernel:
                w[:] = 0
        w.tofile(os.path.join(d, f"{name}_kernel.bin")); b.tofile(os.path.join(d, f"{name}_bias.bin"))
        lines += [f"{name}_kernel {k} {n}", f"{name}_bias {n}"]
    open(os.path.join(d, "shapes.txt"), "w").write("\n".join(lines) + "\n")
    return d
