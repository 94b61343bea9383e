"""Inputs and float64 models for the tests of the sampling and compositing kernels (sampling_kernels.hip: k_stratified, k_resample,
k_composite) away from the shipped 64 + 128 shape: tests/test_sampling_cases_cpu.py shows, with the oracle alone, that these inputs are fit
for purpose; tests/test_gpu_sampling_shapes.py runs them through the kernels.  No GPU in here.

Every ray is generated from its own random stream (BASE_SEED, family, n, ray index): ray r of a family is the same ray whatever the number
of rays asked for, so what the CPU test shows about a family holds for every prefix the GPU tests use."""
import numpy as np

f32 = np.float32
NEAR, FAR = 2.0, 6.0
BASE_SEED = 20261030               # chosen so that tests/test_sampling_cases_cpu.py's conditions hold (nine rays are few: not every seed mixes them)
CUT = 1e-4                      # compute_weights' early break (src/lib.rs:273-279)
NEAR_CUT_REL = 1e-3             # a ray is "near-cut" if its float64 transmittance comes this close (relative) to CUT at or before the cut
U_MAX = f32(1.0 - 2.0 ** -23)   # the largest value (x >> 9) * 2^-23 can take

# (nc, nf) of the resample tests: sort width P = pow2 >= nc + nf (registers up to 256, LDS above), how full it is, trips of the 64-lane loops
RESAMPLE_SHAPES = [(3, 1), (3, 5), (4, 4), (5, 11), (9, 8), (20, 12), (33, 31), (63, 2), (64, 64), (65, 63), (64, 128), (128, 128),
                   (129, 127), (64, 193), (100, 200), (256, 256), (3, 1021), (513, 1), (200, 824), (70, 1000), (1024, 1024)]
RESAMPLE_RAYS = 9               # a workgroup of k_resample holds four rays: two full groups and one ray of a third
COMPOSITE_RAYS = [1, 63, 64, 65, 130]                          # a wave of k_composite holds 64 rays
COMPOSITE_N = [1, 2, 15, 16, 17, 31, 32, 33, 192, 257, 1070]   # it stages 16 samples at a time
PIXELS = [0, 1, 2 ** 24 + 3, 2 ** 32 - 1]                      # Philox counter word 0
SEEDS = [7, 2 ** 32 + 5, 2 ** 63 + 11]                         # Philox key: both halves


def pow2_at_least(v):
    p = 2
    while p < v:
        p <<= 1
    return p


def _rng(family, n, r):
    return np.random.default_rng([BASE_SEED, family, n, r])


def stratified_t(oracle, R, n, family=0):
    """(R, n) strictly ascending sample positions: the oracle's own stratified samples of R distinct pixels."""
    return np.stack([oracle.stratified_samples(BASE_SEED + family, 1000 * n + r, NEAR, FAR, n) for r in range(R)])


def _bumps(rng, t):
    s = np.zeros(t.shape, np.float64)
    for _ in range(int(rng.integers(1, 4))):
        c, wd = rng.uniform(2.3, 5.7), rng.uniform(0.05, 0.8)
        amp = np.exp(rng.uniform(np.log(0.5), np.log(300.0)))
        s += amp * np.exp(-0.5 * ((t.astype(np.float64) - c) / wd) ** 2)
    return s * (rng.uniform(size=t.shape) < 0.7)


def density_rays(oracle, R, n):
    """1-3 Gaussian bumps of density along t, times a random 70 % keep mask; every fourth ray empty.  -> t, sigma (R, n) f32."""
    t = stratified_t(oracle, R, n, 1)
    s = np.zeros((R, n), f32)
    for r in range(R):
        if r % 4 != 3:
            s[r] = _bumps(_rng(1, n, r), t[r]).astype(f32)
    return t, s


def one_hot_positions(n):
    """Sample indices a one-hot ray's surface takes: 0, the last sample, both sides of every multiple of 16 (so of 64 too); n = no surface."""
    ks = {0, n - 1, n}
    for m in range(16, n, 16):
        ks.update((m - 1, m))
    return sorted(ks)


def one_hot_rays(oracle, R, n, offset=0):
    """sigma = 0 in front of sample k_r and 1e12 from k_r on: alpha is exactly 0 or 1 under any correct expf, the weights are exactly
    one-hot (all zero for k_r = n: an empty ray).  Ray r takes position (offset + r) of one_hot_positions(n), cyclically.
    -> t, sigma (R, n) f32, k (R,)"""
    t = stratified_t(oracle, R, n, 2)
    ks = one_hot_positions(n)
    k = np.array([ks[(offset + r) % len(ks)] for r in range(R)])
    s = np.where(np.arange(n)[None, :] >= k[:, None], f32(1e12), f32(0)).astype(f32)
    return t, s, k


def duplicate_rays(oracle, R, n):
    """Density rays in which runs of 2-3 neighbouring t are made equal: zero-width bins, delta = 0, ties in the sort."""
    t = stratified_t(oracle, R, n, 3)
    s = np.zeros((R, n), f32)
    for r in range(R):
        rng = _rng(3, n, r)
        for _ in range(max(1, n // 8)) if n >= 2 else ():
            ln = min(int(rng.integers(2, 4)), n)
            a = int(rng.integers(0, n - ln + 1))
            t[r, a:a + ln] = t[r, a]
        if r % 4 != 3:
            s[r] = _bumps(rng, t[r]).astype(f32)
    assert np.all(np.diff(t, axis=1) >= 0)
    return t, s


WIDE_NC = [4, 9, 33]


def wide_ratio_rays(R, n):
    """Rays whose neighbouring t differ by a factor 2.2 ... 4 (the last at 5.9), densities of optical depth 0 ... 1.5 per interval, every
    fourth ray empty.  For the choice of the bin of a draw that sits ON an edge cdf[j]: the first matching bin j gives
    bins[j] + (bins[j+1] - bins[j]) * 0 = bins[j]; the bin below gives bins[j-1] + (bins[j] - bins[j-1]) * 1, which is bins[j] again
    whenever that subtraction is exact -- always, for neighbours within a factor 2 (Sterbenz), so on evenly spaced samples no test can
    tell the two apart.  Here the subtraction rounds and some edges give another float (tests/test_sampling_cases_cpu.py counts them)."""
    t = np.zeros((R, n), f32); s = np.zeros((R, n), f32)
    for r in range(R):
        rng = _rng(6, n, r)
        tt = 5.9 / np.concatenate([np.cumprod(rng.uniform(2.2, 4.0, size=n - 1))[::-1], [1.0]])
        t[r] = tt.astype(f32)
        if r % 4 != 3:
            d = np.diff(np.concatenate([tt, [FAR]]))
            s[r] = (rng.uniform(0, 1.5, size=n) * (rng.uniform(size=n) < 0.7) / d).astype(f32)
    return t, s


def edges_that_tell_bins_apart(t):
    """(R, n - 3) bool: interior edges j = 1 ... n - 3 at which bins[j-1] + (bins[j] - bins[j-1]) differs from bins[j] in f32"""
    bins = (f32(0.5) * (t[:, :-1] + t[:, 1:])).astype(f32)
    bl, bu = bins[:, :-1], bins[:, 1:]
    return ((bl + (bu - bl).astype(f32)).astype(f32) != bu)[:, :-1] if t.shape[1] > 3 else np.zeros((len(t), 0), bool)


FAMILIES = {"density": density_rays, "one_hot": lambda o, R, n: one_hot_rays(o, R, n)[:2], "duplicate": duplicate_rays}


def explicit_uniforms(cdf, nf, r=0):
    """nf uniforms for a ray with the given CDF (cdf[0] = 0 ... cdf[m] = 1): 0, the largest value the generator returns, values no bin
    matches (1.0, -0.5, 2.0: the reference falls back to the last bin), every bin edge cdf[j] and the float just below it, and a
    regular grid.  Where nf is too small for all of them, ray r starts r * nf entries further into the list: neighbouring rays cover it together."""
    cdf = np.asarray(cdf, f32)
    edges = np.stack([cdf, np.nextafter(cdf, f32(-np.inf))], axis=1).reshape(-1)
    pool = np.concatenate([np.array([0.0, U_MAX, 1.0, -0.5, 2.0], f32), edges]).astype(f32)
    n_grid = nf // 4 if nf >= 16 else 0
    n_pool = nf - n_grid
    if n_pool >= len(pool):
        n_grid, n_pool = nf - len(pool), len(pool)
    head = pool[(r * n_pool + np.arange(n_pool)) % len(pool)]
    grid = ((np.arange(n_grid) + 0.5) / max(n_grid, 1)).astype(f32)
    u = np.concatenate([head, grid]).astype(f32)
    return u[_rng(4, nf, r).permutation(nf)]   # lane order must not matter


def weights_f64(sigma, t, far=FAR):
    """compute_weights (src/lib.rs:250-283) in float64: the same recurrence, the same cut.
    -> w (n,), near_cut (the transmittance came within NEAR_CUT_REL of the cut at or before it), terminated"""
    s = np.asarray(sigma, np.float64); t = np.asarray(t, np.float64)
    n = len(t)
    w = np.zeros(n)
    T, near, cut = 1.0, False, False
    for i in range(n):
        delta = max((t[i + 1] if i + 1 < n else far) - t[i], 0.0)
        alpha = 1.0 - np.exp(-s[i] * delta)
        w[i] = T * alpha
        T *= 1.0 - alpha
        near = near or abs(T - CUT) <= NEAR_CUT_REL * CUT
        if T < CUT:
            cut = True
            break
    return w, near, cut


def integrate_f64(rgb, sigma, t, far=FAR):
    """integrate_ray (src/lib.rs:176-195) in float64 -> (3,)"""
    w, _, _ = weights_f64(sigma, t, far)
    c = np.asarray(rgb, np.float64)
    return (c * w[:, None]).sum(0) + (1.0 - w.sum())


def near_cut_mask(sigma, t, far=FAR):
    return np.array([weights_f64(sigma[r], t[r], far)[1] for r in range(len(t))], bool)


def distinct_colours(R, n):
    """A different, exactly representable colour for every (ray, sample, channel): (1 + index) * 2^-20 (R * n * 3 < 2^20)."""
    assert R * n * 3 < 2 ** 20
    return ((1 + np.arange(R * n * 3, dtype=np.float64)) * 2.0 ** -20).astype(f32).reshape(R, n, 3)
