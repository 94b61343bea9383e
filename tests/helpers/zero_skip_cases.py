"""What the zero-step-skip tests share (test_gpu_zero_skip.py, test_gpu_zero_skip_kernels.py, test_zero_skip_cases_cpu.py): the engineered
networks, the point batches and a float64 bracket of how many ReLU k-steps a batch can execute.  Nothing here needs a GPU.

Cases (all start from fold_utils.write_random_net(..., 20240)):
  a  dense2: all but two units dead -> dense3's k-steps are skipped in long runs, whole chunks of them
  b  dense3 entirely dead -> all 128 k-steps of dense4 (16 chunks; the ring has 3 slots) are skipped
  c  dense0 = raw x on every unit: x < 0 kills all of dense0's outputs, x > 0 keeps them (waves of one workgroup skip differently)
  d  dense7 entirely dead: the alpha head and viewdirs' see zeros
  e  "subnormal": dense6 dead, so dense7's pre-activation IS its bias -- subnormal values of both signs, both zeros, the largest and the
     smallest subnormal -- and a 2^120 alpha kernel brings their ReLU'd sum back into sight: sigma = 2^120 sum max(b7, 0) at every point
  f  "half-space empty": case c without dense5's skip connection and with the alpha bias lowered until sigma is exactly 0 on the whole
     half-space x < 0 (with the skip connection the point's encoding re-enters at dense5 and sigma is no constant there)"""
import os

import numpy as np

from fold_utils import ROW_OF, raw_tensors

DEAD = -1.0e3  # a bias no pre-activation of these networks comes near: |w . x| stays below 1e2 on the test points
N_MAX = 4096
CASES = "abcdef"
# render windows of the 800 x 800 lego camera (x0, y0, w, h).  The camera looks down -y from x = -0.054 with +x on its left: columns right of
# the centre see x < 0 alone, columns left of it cross into x > 0 inside [near, far] -- cases c and f have dead and live rays in one window.
# 21 x 13: a pass and a staging ring end inside a tile.
WINDOWS = {"24x16": (388, 392, 24, 16), "21x13": (391, 395, 21, 13)}
# case f has density from x = 0.04 on: its window reaches 64 columns to the left of the centre (x = 0.29 at far) and 16 to the right
F_WINDOW = (336, 397, 80, 5)
EPS = 1e-3     # kstep_bracket: > 6 x the worst-case f32 rounding of a 319-term dot product at these magnitudes (319 * 2^-24 * 8 = 1.5e-4)


def _edit(d, name, fn):
    path = os.path.join(d, name + ".bin")
    a = np.fromfile(path, dtype="<f4")
    fn(a)
    a.astype("<f4").tofile(path)


def _copy_net(src, dst):
    os.makedirs(dst)
    for f in os.listdir(src):
        with open(os.path.join(src, f), "rb") as i, open(os.path.join(dst, f), "wb") as o:
            o.write(i.read())
    return dst


def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def uniform_points():
    """The 4096 uniform points and unit directions of test_gpu_zero_skip.py."""
    rng = np.random.default_rng(4711)
    return rng.uniform(-2.2, 2.2, size=(3, N_MAX)).astype(np.float32), _dirs(rng, N_MAX)


def _sign_points(rng):
    """Case (c): x < 0 kills every unit of dense0, x > 0 keeps them.  First half: waves 0-1 of every 128-point workgroup tile dead and
    waves 2-3 live; second half: alternating per 32 points (per wave).  The prefixes n = 128, 129 end inside / just behind a tile."""
    pts = rng.uniform(-2.2, 2.2, size=(3, N_MAX)).astype(np.float32)
    i = np.arange(N_MAX)
    live = np.where(i < N_MAX // 2, (i // 64) % 2 == 1, (i // 32) % 2 == 1)
    pts[0] = np.where(live, 1.0, -1.0) * np.maximum(np.abs(pts[0]), 0.05)
    return pts.astype(np.float32), live


def case_points(case):
    """-> (points (3, 4096), directions (4096, 3), live or None): the sign points for the two networks that follow the sign of x."""
    pts, dirs = uniform_points()
    if case in "cf":
        pts, live = _sign_points(np.random.default_rng(99))
        return pts, dirs, live
    return pts, dirs, None


def ray_points(n_rays=128, n_samples=32, seed=7):
    """A ray-ordered batch: rays from one origin outside the unit box towards random targets inside it, n_samples equally spaced samples
    on each (t = 2 .. 6 along the unit direction), ray after ray -- with 32 samples a wave holds exactly one ray, and its 32 points lie
    close together the way a render's do.  -> (points (3, n), directions (n, 3))."""
    rng = np.random.default_rng(seed)
    origin = np.array([-0.05, 3.85, 1.2])
    d = rng.uniform(-1.0, 1.0, size=(n_rays, 3)) - origin
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.linspace(2.0, 6.0, n_samples)
    p = origin[None, None, :] + d[:, None, :] * t[None, :, None]
    return np.ascontiguousarray(p.reshape(-1, 3).T, dtype=np.float32), np.repeat(d, n_samples, axis=0).astype(np.float32)


# the ten values of poisoned_points, as bit patterns: +NaN, a NaN with the sign bit set, +inf, -inf, 1e30, -1e30, 3e38, 2049.0 (just outside
# the documented input domain), the smallest subnormal and -0.0
POISON_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000], np.uint32)
POISON = np.concatenate([POISON_BITS.view(np.float32), np.array([1e30, -1e30, 3e38, 2049.0, 1e-45, -0.0], np.float32)])
# two in one wave (64, 70), one among a wave's first sixteen points (5), the last point, the rest spread over the batch
POISON_AT = np.array([64, 70, 5, N_MAX - 1, 1000, 1777, 2079, 3000, 3500, 200])


def poisoned_points():
    """The uniform points with one coordinate replaced at ten of them -> (points, directions, poisoned (4096,) bool)."""
    pts, dirs = uniform_points()
    pts = pts.copy()
    for k, (i, v) in enumerate(zip(POISON_AT, POISON)):
        pts[k % 3, i] = v
    hit = np.zeros(N_MAX, bool)
    hit[POISON_AT] = True
    return pts, dirs, hit


SUBNORMAL_HEAD = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32)   # +-0, +-1e-45, +-1.1754942e-38


def subnormal_bias():
    """dense7_bias of case e: 256 values with random signs in +-[1e-41, 1e-39]; the first eight are +0.0, -0.0, +-1e-45 (the smallest
    subnormal), +-1.1754942e-38 (the largest) and +-1e-40."""
    rng = np.random.default_rng(1)
    b = (rng.uniform(1e-41, 1e-39, size=256) * rng.choice([-1.0, 1.0], size=256)).astype(np.float32)
    b[:6] = SUBNORMAL_HEAD.view(np.float32)
    b[6:8] = np.array([1e-40, -1e-40], np.float32)
    return b


def subnormal_sigma_fp64():
    """sigma of case e at every point: 2^120 * sum max(b7, 0), in float64 (every term and the sum are exact there)."""
    return float(2.0 ** 120 * np.maximum(subnormal_bias().astype(np.float64), 0).sum())


def _make_case(case, base, tmp, oracle=None):
    """-> (directory, twin directory or None): the twin differs only in weights the engineered zeros make irrelevant.  Case f needs the
    oracle (one evaluation of case c at a point with x < 0)."""
    d = _copy_net(base, str(tmp / case))
    twin = str(tmp / (case + "_twin"))
    if case == "a":       # dense2: all but two units dead -> dense3's k-steps skipped in long runs, whole chunks of them
        keep = [37, 201]
        def bias(b):
            k = b[keep].copy(); b[:] = DEAD; b[keep] = k
        _edit(d, "dense2_bias", bias)
        _copy_net(d, twin)
        def rows(w):
            w = w.reshape(256, 256); k = w[keep].copy(); w[:] = 0; w[keep] = k
        _edit(twin, "dense3_kernel", rows)
    elif case == "b":     # dense3 entirely dead -> all 128 k-steps (16 chunks, the ring has 3 slots) of dense4 skipped
        _edit(d, "dense3_bias", lambda b: b.__setitem__(slice(None), DEAD))
        _copy_net(d, twin)
        _edit(twin, "dense4_kernel", lambda w: w.__setitem__(slice(None), 0))
    elif case in "cf":    # dense0 = raw x on every unit (reference feature 0): relu(h0) = max(x, 0) for all 256 units
        def kern(w):
            w = w.reshape(63, 256); w[:] = 0; w[0] = 1.0
        _edit(d, "dense0_kernel", kern)
        _edit(d, "dense0_bias", lambda b: b.__setitem__(slice(None), 0))
        if case == "c":
            _copy_net(d, twin)
            _edit(twin, "dense1_kernel", lambda w: w.__setitem__(slice(None), 0))
        else:
            # x < 0: nothing of the point may be left behind dense0, so dense5's skip connection (its 63 encoding rows) goes too; the
            # density's pre-activation is then one constant there, and a function of x alone elsewhere, rising from that constant by 0.02 at
            # x = 0.05 and by 1 at x = 2.2.  Scaled by 64 and lowered by the constant plus 1 it is -1 on x < 0 and positive from x = 0.04 on.
            def skip_rows(w):
                w.reshape(319, 256)[:63] = 0
            _edit(d, "dense5_kernel", skip_rows)
            _edit(d, "alpha_kernel", lambda w: w.__setitem__(slice(None), w * np.float32(64.0)))
            _edit(d, "alpha_bias", lambda b: b.__setitem__(slice(None), 0))
            p = np.array([[-1.0], [0.3], [-0.4]], np.float32)
            const = float(oracle.Net(d).forward_batch(p, np.array([[0.0, 0.0, 1.0]], np.float32))[1][0])
            assert const > 1.0                                          # positive, hence the pre-activation itself and not its ReLU
            _edit(d, "alpha_bias", lambda b: b.__setitem__(slice(None), np.float32(-(const + 1.0))))
            twin = None
    elif case == "d":     # dense7 entirely dead: the alpha head and viewdirs' see zeros
        _edit(d, "dense7_bias", lambda b: b.__setitem__(slice(None), DEAD))
        twin = None
    elif case == "e":     # dense6 dead -> dense7's 128 k-steps dead and its outputs = its subnormal biases; alpha = 2^120 sum relu(.)
        _edit(d, "dense6_bias", lambda b: b.__setitem__(slice(None), DEAD))
        _edit(d, "dense7_bias", lambda b: b.__setitem__(slice(None), subnormal_bias()))
        _edit(d, "alpha_kernel", lambda w: w.__setitem__(slice(None), np.float32(2.0 ** 120)))
        _edit(d, "alpha_bias", lambda b: b.__setitem__(slice(None), 0))
        twin = None
    else:
        raise ValueError(case)
    return d, twin


def check_case(case, oracle, d, twin, pts, dirs, live):
    """Assert from the oracle's outputs (and float64) that the engineered condition of a case holds on its points -> (rgb, sigma)."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    ergb, esg = oracle.Net(d).forward_batch(pts, dirs)
    assert np.isfinite(esg).all() and np.isfinite(ergb).all()
    if case == "d":
        assert np.all(esg == np.float32(0.7))                      # sigma = relu(alpha bias): nothing of the point reaches the head
    elif case == "e":
        want = subnormal_sigma_fp64()                              # a path that flushes subnormals returns 0 instead
        assert np.all(np.abs(esg - want) <= 1e-6 * want) and np.all(esg > 0.01), (esg.min(), esg.max(), want)
    elif case == "f":
        assert np.all(esg[~live] == 0) and (esg[live] > 0).mean() >= 0.25, (esg[~live].max(), (esg[live] > 0).mean())
    else:
        trgb, tsg = oracle.Net(twin).forward_batch(pts, dirs)
        same = np.all(bits(trgb) == bits(ergb), axis=1) & (bits(tsg) == bits(esg))
        if case == "c":                                            # dense1's kernel is irrelevant exactly where x < 0
            assert np.all(same[~live]) and same[live].mean() < 0.01
        else:                                                      # the consumer's rows of the dead units are irrelevant everywhere
            assert np.all(same)
    assert ergb.std() > 1e-3 and (case in "de" or esg.std() > 0)   # ... and the network still computes something
    return ergb, esg


# ---- float64 bracket of the executed ReLU k-steps ------------------------------------------------------------------------------------
def preacts_fp64(d, pts):
    """The pre-activations of dense0..7 at pts (3, n) in float64 from the raw tensors -> list of eight (n, 256) arrays.  The encoding as in
    test_gpu_parity.py _forward_fp64: arguments float32(2^k) * p."""
    W = raw_tensors(d)
    v = np.asarray(pts, np.float32).T
    e = [v.astype(np.float64)]
    for k in range(10):
        a = (np.float32(2.0 ** k) * v).astype(np.float64)
        e += [np.sin(a), np.cos(a)]
    e = np.concatenate(e, axis=1)
    pre, h = [], e
    for i in range(8):
        if i == 5:
            h = np.concatenate([e, h], axis=1)
        z = h @ W[f"dense{i}_kernel"] + W[f"dense{i}_bias"]
        pre.append(z)
        h = np.maximum(z, 0)
    return pre


# unit of k-step s (0..127) on lane half 0 / 1: tile s >> 4, register s & 15 (mlp_layout.h regFeature)
STEP_UNITS = np.array([[32 * (s >> 4) + ROW_OF[s & 15][h] for h in (0, 1)] for s in range(128)])


def n_waves(n):
    """Waves of 32 points that a launch over n points runs: whole 128-point workgroup tiles, padding slots repeat the last point."""
    return 4 * ((n + 127) // 128)


def pad_to_waves(a, axis):
    """Repeat the last point along `axis` up to a whole number of workgroup tiles, as the kernels' clamped loads do."""
    n = a.shape[axis]
    idx = np.minimum(np.arange(32 * n_waves(n)), n - 1)
    return np.take(a, idx, axis=axis)


def kstep_bracket(pre_list, eps=EPS):
    """(certain_live, certain_dead, total) ReLU k-steps summed over (wave of 32 consecutive points, layer of pre_list, k-step 0..127).  Step s
    reads units STEP_UNITS[s] over the wave's 32 points: certainly live if one of those 64 pre-activations is above +eps, certainly dead
    if all of them are below -eps.  The full kernel has 8 ReLU-input layers per wave (the outputs of dense0..7: they feed dense1..4, the
    hidden rows of dense5, dense6, dense7 and viewdirs'), the sigma-only kernels the first 7."""
    live = dead = total = 0
    for z in pre_list:
        z = pad_to_waves(z, 0)
        w = z.reshape(-1, 32, 256)[:, :, STEP_UNITS]            # (waves, 32 points, 128 steps, 2 units)
        hi = w.max(axis=(1, 3)); lo = w.min(axis=(1, 3))
        assert not (np.isnan(hi).any() or np.isnan(lo).any())
        live += int((hi > eps).sum()); dead += int((hi < -eps).sum()); total += hi.size
    return live, dead, total


def dead_wave_steps(live_points):
    """Case c / f: 128 x the number of waves all of whose 32 points (padding included) have x <= 0 -- every k-step of dense1 is dead there."""
    w = pad_to_waves(np.asarray(live_points, bool), 0).reshape(-1, 32)
    return 128 * int((~w.any(axis=1)).sum())
