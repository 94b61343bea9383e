"""CPU tests of the folded image the f32 kernels read (host_util.cpp fold_network; mlp_layout.h kChunksFullFolded): the bottleneck
layer has no activation (src/network.rs:218) and feeds only the viewdirs layer, so the loader replaces the two by
W' = W_b . W_v[0:256], b' = b_v + b_b^T . W_v[0:256].  Checked here without a device: the image's shape and what it shares with
the packed image, the exactness of W' and b' against a float64 product of the raw tensors, and a lane-by-lane walk of the folded
stream as mlp_kernel.hip consumes it, against the reference's golden scalars and the oracle."""
import os

import numpy as np
import pytest

from conftest import SCENE
from fold_utils import (AW, BIAS, BIASV, CHUNK, H_, LANE, MISC, N_FOLDED, N_PACKED, N_SIGMA, P_, ROW_OF, RW, fold_fp64, image,
                        unpermute_folded, write_random_net)


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_folded_image_shape_and_shared_content(native, which):
    d = os.path.join(SCENE, which)
    ws, sm = image(native, d, folded=False)
    fws, fsm = image(native, d, folded=True)
    assert ws.size == N_PACKED * CHUNK and fws.size == N_FOLDED * CHUNK and fsm.size == sm.size
    assert fws[:N_SIGMA * CHUNK].tobytes() == ws[:N_SIGMA * CHUNK].tobytes()                  # dense0..7: untouched
    assert fws[(N_FOLDED - 1) * CHUNK:].tobytes() == ws[(N_PACKED - 1) * CHUNK:].tobytes()    # the dir-encoding chunk of viewdirs
    outside = np.ones(sm.size, bool); outside[BIASV:BIASV + 128] = False
    assert fsm[outside].tobytes() == sm[outside].tobytes()                                    # only the viewdirs bias slot moves
    assert not np.array_equal(fsm[BIASV:BIASV + 128], sm[BIASV:BIASV + 128])                  # ... and it does (b_b != 0 in lego)


def _assert_half_ulp(got, want64):
    """|got - want| <= 2^-24 |want| (1 + 1e-6): half an f32 ulp, plus room for the order of an fp64 summation."""
    err = np.abs(got.astype(np.float64) - want64)
    bound = 2.0 ** -24 * np.abs(want64) * (1 + 1e-6)
    assert (err <= bound).all(), (float((err / np.maximum(bound, 1e-300)).max()), int((err > bound).sum()))


@pytest.mark.parametrize("case", ["coarse", "fine", "random, large bottleneck bias", "zero bottleneck kernel"])
def test_fold_is_the_fp64_product_rounded_once(native, tmp_path, case):
    if case in ("coarse", "fine"):
        d = os.path.join(SCENE, case)
    else:
        d = write_random_net(tmp_path / "net", 20240, zero_bottleneck_kernel=case.startswith("zero"))
    Wf, bf = unpermute_folded(*image(native, d, folded=True))
    W64, b64 = fold_fp64(d)
    assert Wf.dtype == np.float32 and W64.shape == (256, 128) and b64.shape == (128,)
    _assert_half_ulp(Wf, W64)
    _assert_half_ulp(bf, b64)
    if case.startswith("zero"):
        assert not Wf.any()                                              # W_b = 0: the head sees b' = b_v + b_b^T W_v alone
        assert np.abs(b64).max() > 1.0                                   # ... and that bias is not a small thing here
    else:
        assert np.abs(Wf).max() > 0.01 and np.abs(W64).max() > 0.01


def test_fold_under_host_sanitizers(tmp_path):
    """fold_network in the stand-alone sanitizer build of the host-only sources (`make host-asan`: AddressSanitizer + UBSan, no HIP, no
    Python in the process): the lego networks, a zero bottleneck kernel, and a directory the loader refuses."""
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "nerf-rs_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "host-asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=87", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    zero = write_random_net(tmp_path / "zero", 20240, zero_bottleneck_kernel=True)
    for d, want in ((os.path.join(SCENE, "coarse"), 0), (os.path.join(SCENE, "fine"), 0), (zero, 0), (str(tmp_path / "missing"), -2)):
        p = subprocess.run([os.path.join(csrc, "build", "host_asan_driver"), "debug_fold", d], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, (d, p.stdout[-2000:], p.stderr[-6000:])
        assert f"debug_fold rc={want}" in p.stdout, p.stdout
        if want == 0:
            assert f"folded {N_FOLDED * CHUNK} + 3136 floats" in p.stdout


# ---- a wave walking the folded stream: numpy emulation of the kernel's lane/register layout, as in test_host_logic.py ----------
def _mfma(acc, a, b):
    """v_mfma_f32_32x32x2_f32: A[i=l&31][k=l>>5] = a[l], B[k=l>>5][j=l&31] = b[l]; D reg r of lane l =
    D[(r&3)+8(r>>2)+4(l>>5)][l&31]."""
    D = a.reshape(2, 32).T.astype(np.float64) @ b.reshape(2, 32).astype(np.float64)
    acc += D[ROW_OF[:, H_], P_[None, :]]


def _emulate_wave_folded(ws, sm, pts, dirs):
    """One 32-point wave tile through the full network exactly as mlp_kernel.hip walks the FOLDED stream: dense0..7, alpha, then
    viewdirs' on [relu(h7) ; dir encoding] with bias b', rgb."""
    pos = pts[:, P_]; d = dirs[P_].T
    E = np.zeros((2, 16, 64))
    f0 = np.where(H_ == 1, 32.0, 1.0)
    for o in range(5):
        for ax in range(3):
            arg = np.float32(f0 * 2.0 ** o) * pos[ax]
            for idx, val in ((6 * o + ax, np.sin(np.float64(arg))), (6 * o + 3 + ax, np.cos(np.float64(arg)))):
                E[idx >> 4, idx & 15] = val
    E[1, 14] = np.where(H_ == 1, pos[2], pos[0]); E[1, 15] = np.where(H_ == 1, 0.0, pos[1])
    cur = [0]

    def bias(off, nt):
        return np.stack([sm[off + (t * 2 + H_) * 16 + r] for t in range(nt) for r in range(16)]).reshape(nt, 16, 64).astype(np.float64)

    def steps(inp, out, relu):  # one input tile (16 k-steps)
        nt = out.shape[0]
        for r in range(16):
            b = np.maximum(inp[r], 0) if relu else inp[r]
            for g in range(nt // 4):
                piece = ws[cur[0]: cur[0] + 256].reshape(64, 4); cur[0] += 256
                for q in range(4):
                    _mfma(out[4 * g + q], piece[:, q], b)

    X = bias(BIAS, 8); steps(E[0], X, False); steps(E[1], X, False)
    for layer in range(1, 5):
        Y = bias(BIAS + layer * 256, 8)
        for t in range(8):
            steps(X[t], Y, True)
        X = Y
    Y = bias(BIAS + 5 * 256, 8); steps(E[0], Y, False); steps(E[1], Y, False)
    for t in range(8):
        steps(X[t], Y, True)
    X = Y
    for layer in (6, 7):
        Y = bias(BIAS + layer * 256, 8)
        for t in range(8):
            steps(X[t], Y, True)
        X = Y
    assert cur[0] == N_SIGMA * CHUNK
    aw = np.stack([sm[AW + H_ * 128 + k] for k in range(128)]).reshape(8, 16, 64)
    part = (aw * np.maximum(X, 0)).sum(axis=(0, 1))
    sigma = np.maximum(part + part[LANE ^ 32] + sm[MISC], 0)
    D = np.zeros((16, 64))
    f = np.where(H_ == 1, 4.0, 1.0)
    for o in range(2):
        for ax in range(3):
            arg = np.float32(f * 2.0 ** o) * d[ax]
            D[6 * o + ax] = np.sin(np.float64(arg)); D[6 * o + 3 + ax] = np.cos(np.float64(arg))
    for ax in range(3):
        D[12 + ax] = np.where(H_ == 1, 0.0, d[ax])
    V = bias(BIASV, 4)                       # b'
    for t in range(8):
        steps(X[t], V, True)                 # W' on relu(h7): no bottleneck layer in between
    steps(D, V, False)
    assert cur[0] == N_FOLDED * CHUNK == ws.size
    rgb = np.zeros((3, 64))
    for c in range(3):
        rw = np.stack([sm[RW + (H_ * 3 + c) * 64 + k] for k in range(64)]).reshape(4, 16, 64)
        part = (rw * np.maximum(V, 0)).sum(axis=(0, 1))
        rgb[c] = 1.0 / (1.0 + np.exp(-(part + part[LANE ^ 32] + sm[MISC + 1 + c])))
    return rgb[:, :32].T, sigma[:32]


@pytest.mark.parametrize("which", ["coarse", "fine"])
def test_folded_stream_reproduces_the_network(native, oracle, samples, oracle_nets, which):
    """test_host_logic.py's 32 points (the 15 golden-scalar points + 17 random ones) and its bounds, on the folded image."""
    ws, sm = image(native, os.path.join(SCENE, which), folded=True)
    assert ws.size == N_FOLDED * CHUNK and sm.size % 64 == 0
    origin = np.float32(samples["camera_origin"]); z = np.float32(samples["z_vals"])
    pts = np.zeros((3, 32), np.float32); dirs = np.zeros((32, 3), np.float32); dirs[:, 2] = 1
    exp_s, exp_c = [], []
    for e, ex in enumerate(samples["examples"]):
        rd = np.float32(ex["ray_d"])
        pts[:, 5 * e: 5 * e + 5] = origin[:, None] + rd[:, None] * z[None, :]
        dirs[5 * e: 5 * e + 5] = np.float32(ex["viewdir_unit"])
        exp_s += ex[f"{which}_sigma"]; exp_c += ex[f"{which}_rgb"]
    rng = np.random.default_rng(1)
    pts[:, 15:] = rng.uniform(-2.2, 2.2, size=(3, 17)); v = rng.normal(size=(17, 3))
    dirs[15:] = v / np.linalg.norm(v, axis=1, keepdims=True)
    rgb, sigma = _emulate_wave_folded(ws, sm, pts, dirs)
    exp_s, exp_c = np.float32(exp_s), np.float32(exp_c)
    print(f"\n{which}: max |rgb - golden| {np.abs(rgb[:15] - exp_c).max():.2e}")
    assert np.all(np.abs(sigma[:15] - exp_s) <= 1e-4 * (1 + np.abs(exp_s)))      # the reference's golden scalars
    assert np.all(np.abs(rgb[:15] - exp_c) <= 1e-5)
    o_rgb, o_sig = oracle_nets[0 if which == "coarse" else 1].forward_batch(pts, dirs)
    print(f"{which}: max |rgb - oracle| {np.abs(rgb - o_rgb).max():.2e}")
    assert np.all(np.abs(sigma - o_sig) <= 1e-4 * (1 + np.abs(o_sig))) and np.all(np.abs(rgb - o_rgb) <= 1e-5)
