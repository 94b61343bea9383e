"""Inputs and plain float64 models for the stage tests of certify_zero's device pieces (sampling_kernels.hip k_cert_plan, k_cert_verify,
k_cert_audit; the ray-sequential 16-bit pre-filter of mlp_kernel_bf16v2.hip): tests/test_certify_cases_cpu.py shows that the inputs are
fit for purpose, tests/test_gpu_certify_stages.py runs them through nerf_stage_cert_* / nerf_stage_prefilter.  NumPy only, no GPU.

The models state the CONTRACT (include/nerf_mi355x.h), per sample and per ray; they know nothing of waves, groups of 64, staging areas or
atomics.  Index sets are sets: the order of a list is arbitrary by design."""
import os

import numpy as np

f32 = np.float32
U32 = 0xFFFFFFFF
NOT_EVALUATED = np.array([U32], np.uint32).view(f32)[0]     # the pre-filter's "not evaluated" pattern (a NaN)
CUT = 1e-4                                                  # compute_weights' early break (src/lib.rs:273-279)
STAGE = 256                                                 # audited certificates per run of rays_per_wave consecutive rays
# mirrored from nerf_internal.h (nerf_ctx defaults): predicted cut at optical depth 9.6, one certificate in 128 audited, one in 16 of those
# within twice the margin, "probably zero" below -margin x 0.1; floors of the margins with the f16 / bf16 pre-filter (coarse, fine)
DEPTH_LIMIT, MASK, MASK_NEAR, ZERO_FRAC = f32(9.6), 127, 15, f32(0.1)
FLOORS_F16, FLOORS_BF16 = (0.25, 0.5), (1.0, 3.0)

PLAN_SPR = [1, 2, 63, 64, 65, 192, 255, 256, 257, 513, 800, 1070]   # groups of 64, batches of 256, rays_per_wave 8 (<= 768), 7 (800), 5 (1070)
PLAN_RAYS = [1, 2, 31, 32, 33, 65]                                   # one ray either side of a workgroup of 4 waves x 8 rays
VERIFY_JSTAR = [0, 1, 63, 64, 65]                                    # and spr itself
OVERFLOW_RUNS = 4                                                    # family D: this many full runs of rays_per_wave rays and one ray more
GUARD_CAP = 0.02                                                     # at most this share of a smooth family may be left out


def rays_per_wave(spr):
    """What launch_cert_plan chooses (96 KiB of staging for four waves, at most 8 rays): compared with the stage call's own answer."""
    return max(1, min(8, (96 * 1024) // (16 * spr)))


def audit_pick(idx, salt, mask):
    """The documented pick: ((idx ^ salt) * 0x9E3779B1 mod 2^32) >> 7 & mask == 0."""
    x = (np.asarray(idx, np.uint64) ^ np.uint64(salt)) * np.uint64(0x9E3779B1) & np.uint64(U32)
    return ((x >> np.uint64(7)) & np.uint64(mask)) == 0


def deltas(t, far):
    t = np.asarray(t, np.float64)
    return np.maximum(np.concatenate([t[:, 1:], np.full((len(t), 1), float(far))], axis=1) - t, 0.0)


def depth_in_front(pre, t, far):
    """(R, spr) float64: sum over the samples in front of i of max(pre, 0) max(delta, 0) (a NaN pre-activation adds nothing)."""
    p = np.asarray(pre, np.float64)
    with np.errstate(invalid="ignore"):
        od = np.where(p > 0, p, 0.0) * deltas(t, far)
    c = np.cumsum(od, axis=1)
    return np.concatenate([np.zeros((len(c), 1)), c[:, :-1]], axis=1)


def plan_model(pre, t, far, margin, depth_limit, mask=MASK, mask_near=MASK_NEAR, salt=0, zero_threshold=None, pick_shift=0, cut_early=0,
               near_inclusive=False):
    """-> dict of per-ray / per-sample facts.  The last three arguments make MUTANTS (a pick fraction 2^-pick_shift of the contract's, a
    cut `cut_early` samples early, a near band that includes -2 margin) for tests/test_certify_cases_cpu.py."""
    pre = np.asarray(pre, f32); R, spr = pre.shape
    m = float(f32(margin))
    p = pre.astype(np.float64)
    with np.errstate(invalid="ignore"):
        before = depth_in_front(pre, t, far)
        beyond = before > float(f32(depth_limit))
        jstar = np.where(beyond.any(1), beyond.argmax(1), spr)
        jstar = np.where(beyond.any(1), np.maximum(jstar - cut_early, 0), jstar)
        certified = (p < -m) & (p >= float(f32(-3.0e38)))
        near = (p >= -2.0 * m) if near_inclusive else (p > -2.0 * m)
        probable_zero = (p < -float(f32(zero_threshold))) if zero_threshold is not None else np.zeros(p.shape, bool)
    unc = ~certified
    front_of_cut = np.arange(spr)[None, :] < jstar[:, None]
    idx = np.arange(R * spr, dtype=np.uint64).reshape(R, spr)
    pick = certified & front_of_cut & np.where(near, audit_pick(idx, salt, (mask_near + 1 << pick_shift) - 1), audit_pick(idx, salt, (mask + 1 << pick_shift) - 1))
    listed_unc = unc & front_of_cut
    back = (listed_unc & probable_zero) if zero_threshold is not None else np.zeros(p.shape, bool)
    return dict(jstar=jstar.astype(np.int32), before=before, uncertain=unc, pick=pick, near=near & certified,
                front=set(idx[listed_unc & ~back].astype(np.int64).tolist()), back=set(idx[back].astype(np.int64).tolist()),
                picks=set(idx[pick].astype(np.int64).tolist()), picks_go_back=zero_threshold is not None,
                marked=unc & ~front_of_cut, buffer=np.where(unc & ~front_of_cut, f32(-1), f32(0)).astype(f32))


def near_limit_rays(before, depth_limit, rel=1e-5):
    """Rays with a float64 prefix depth within `rel` (relative) of the limit: their j* may differ by f32 summation order alone."""
    with np.errstate(invalid="ignore"):
        return (np.abs(before - float(f32(depth_limit))) <= rel * float(f32(depth_limit))).any(1)


def picks_per_run(pick, rpw):
    """Picks of each run of rpw consecutive rays (what one wave stages between two flushes)."""
    per_ray = pick.sum(1)
    return np.array([per_ray[a:a + rpw].sum() for a in range(0, len(per_ray), rpw)])


# ---- plan families ---------------------------------------------------------------------------------------------------------------------
def _grid_t(R, spr, t0=2.0):
    """delta = 2^-6 exactly, far = last sample + 2^-6 (spr <= 1070: every t is a multiple of 2^-6 below 32, exact in f32)."""
    t = (t0 + np.arange(spr) * 2.0 ** -6)[None, :].repeat(R, 0).astype(f32)
    return t, f32(t0 + spr * 2.0 ** -6)


EXACT_LIMIT = f32(0.25)           # 256 units of 2^-10: family A reaches it EXACTLY
EXACT_CUTS = (1, 63, 64, 65, 255, 256, 257)


def _split(units, k, rng):
    """k positive integers summing to `units`."""
    cutpoints = np.sort(rng.choice(np.arange(1, units), size=k - 1, replace=False)) if k > 1 else np.array([], int)
    return np.diff(np.concatenate([[0], cutpoints, [units]])).astype(np.float64)


def exact_sum_rays(R, spr, seed=1):
    """Family A: pre in multiples of 2^-4 within +-32, delta = 2^-6: every term of the depth is a whole number of units of 2^-10 and no sum
    exceeds 257 units, so every partial sum is exact in f32 in ANY order and j* is predicted exactly.  Ray r cuts at sample c = cuts[r % len]
    (1, 63, 64, 65, 255, 256, 257, spr - 1 where they exist; spr = no cut): up to 20 samples in front of c - 1 hold the limit's 256 units
    between them, so the depth in front of sample c - 1 EQUALS the limit (strict >: no cut there), and sample c - 1 adds one unit.  A ray
    without a cut holds exactly the limit in total.  The background is non-positive.  -> t, pre, far, the cuts (R,)"""
    rng = np.random.default_rng([20261020, seed, spr])
    t, far = _grid_t(R, spr)
    cuts = sorted({c for c in EXACT_CUTS + (spr - 1,) if 0 < c < spr}) + [spr]
    pre = (rng.integers(-512, 1, size=(R, spr)) / 16.0).astype(f32)
    want = np.zeros(R, np.int32)
    units = int(float(EXACT_LIMIT) * 1024)
    for r in range(R):
        c = cuts[r % len(cuts)]
        want[r] = c
        room = spr if c == spr else c - 1                # samples that share the limit's units
        if room >= 1:
            k = min(room, 20)
            pos = np.sort(rng.choice(room, size=k, replace=False))
            pre[r, pos] = _split(units, k, rng) / 16.0   # units x 2^-10 / 2^-6
        if c < spr:
            pre[r, c - 1] = (units + 1) / 16.0 if c == 1 else 1.0 / 16.0
    assert np.abs(pre).max() <= 32
    return t, pre, far, want


def smooth_rays(R, spr, seed=3):
    """Family B: the Gaussian-bump densities of sampling_cases.py as pre-activations, shifted so that the gaps are certified, near-margin
    or uncertain; irregular ascending t."""
    from . import sampling_cases as sc
    pre = np.zeros((R, spr), f32); t = np.zeros((R, spr), f32)
    for r in range(R):
        rng = np.random.default_rng([20261020, seed, spr, r])
        tt = np.sort(rng.uniform(sc.NEAR, sc.FAR, size=spr)).astype(f32)
        t[r] = tt
        bump = sc._bumps(rng, tt) if r % 4 != 3 else np.zeros(spr)
        floor = -rng.uniform(0.0, 4.0, size=spr)         # margins of 0.25 ... 3: some below -2 m, some inside the near band, some uncertain
        pre[r] = np.where(bump > 1e-3, bump, floor).astype(f32)
    return t, pre, f32(sc.FAR)


def special_values(margin, zero_threshold):
    m = f32(margin)
    return {"nan": f32(np.nan), "not_evaluated": NOT_EVALUATED, "+inf": f32(np.inf), "-inf": f32(-np.inf), "-0": f32(-0.0),
            "-margin": -m, "just_above_-margin": np.nextafter(-m, f32(0)), "just_below_-margin": np.nextafter(-m, f32(-np.inf)),
            "-2margin": f32(-2) * m, "just_above_-2margin": np.nextafter(f32(-2) * m, f32(0)),
            "-zero_threshold": -f32(zero_threshold), "just_below_-zero_threshold": np.nextafter(-f32(zero_threshold), f32(-np.inf)),
            "-3e38": f32(-3.0e38), "just_below_-3e38": np.nextafter(f32(-3.0e38), f32(-np.inf))}


# what each special value must be: (certified, near band, goes to the back part when listed)
SPECIAL_CLASS = {"nan": (False, None, False), "not_evaluated": (False, None, False), "+inf": (False, None, False), "-inf": (False, None, True),
                 "-0": (False, None, False), "-margin": (False, None, True), "just_above_-margin": (False, None, True),
                 "just_below_-margin": (True, True, None), "-2margin": (True, False, None), "just_above_-2margin": (True, True, None),
                 "-zero_threshold": (False, None, False), "just_below_-zero_threshold": (False, None, True),
                 "-3e38": (True, False, None), "just_below_-3e38": (False, None, True)}


def special_rays(R, spr, margin, zero_threshold, seed=4):
    """Family C: certified background (every index a candidate for the audit), the special values at random positions in front of and
    behind a cut, and two stretches of DESCENDING t (a negative delta adds no depth).  +inf stands behind the cut only when there is
    one (depth inf x delta), never on a zero-width interval (inf x 0)."""
    rng = np.random.default_rng([20261020, seed, spr])
    vals = special_values(margin, zero_threshold)
    names = list(vals)
    t = np.sort(rng.uniform(2.0, 6.0, size=(R, spr)), axis=1).astype(f32)
    pre = (-f32(margin) * rng.uniform(1.01, 4.0, size=(R, spr))).astype(f32)
    where = {}
    for r in range(R):
        if spr >= 8:
            a = int(rng.integers(0, spr - 3))
            t[r, a:a + 3] = t[r, a:a + 3][::-1]                               # descending: delta < 0 twice
        for k, name in enumerate(names):
            if name == "+inf" and spr < 4:
                continue
            i = int(rng.integers(0, spr))
            if name == "+inf":
                i = spr - 1                                                   # the last interval ends at far > every t: delta > 0
            pre[r, i] = vals[name]
            where.setdefault(name, []).append((r, i))
        if r % 2 and spr >= 16:                                               # a cut in the middle: a dense sample of depth >> limit
            pre[r, spr // 2] = f32(1e6)
    return t, pre, f32(6.5), where


def overflow_rays(R, spr, margin):
    """Family D: every sample certified inside the near band (1 in 16 picked): rays_per_wave x spr / 16 > 256 from spr = 513 on."""
    rng = np.random.default_rng([20261020, 5, spr])
    t, far = _grid_t(R, spr)
    pre = (-f32(margin) * rng.uniform(1.05, 1.95, size=(R, spr))).astype(f32)
    return t, pre, far


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
def verify_model(sigma, t, far, jstar, cut_early=0):
    """-> (sigma afterwards, set of listed sample indices, fall-back rays, near-cut rays).  cut_early: the mutant that looks one sample less."""
    s = np.asarray(sigma, f32).copy(); R, spr = s.shape
    d = deltas(t, far)
    listed, fallback = set(), 0
    near = np.zeros(R, bool)
    for r in range(R):
        j = int(jstar[r])
        if j >= spr:
            continue
        T, cut = 1.0, False
        for i in range(max(j - cut_early, 0)):
            T *= np.exp(-float(s[r, i]) * d[r, i])
            near[r] |= abs(T - CUT) <= 1e-3 * CUT
            if T < CUT:
                cut = True
                break
        marks = np.nonzero(s[r, j:] == f32(-1))[0] + j
        s[r, marks] = 0
        if not cut and len(marks):
            listed.update((r * spr + marks).tolist())
            fallback += 1
    return s, listed, fallback, near


def one_hot_verify_rays(spr, seed=6):
    """One ray per (j*, where the exact cut falls, where the marks are): sigma = 0 then 1e12 from sample k on (alpha exactly 0 or 1), so the
    exact cut is AT k: inside the prefix iff k < j*.  k = j* - 1: cleared, no list; k = j*: every mark listed, one fall-back ray; k = spr: no
    cut anywhere.  Marks at j*, at spr - 1, or none.  j* = spr: the ray is left alone (its marks stay)."""
    rng = np.random.default_rng([20261020, seed, spr])
    js = sorted({j for j in VERIFY_JSTAR + [spr] if j <= spr})
    rows = []
    for j in js:
        for k in sorted({j - 1, j, spr} - {-1}):
            for marks in ("at_j", "last", "none", "both"):
                rows.append((j, k, marks))
    R = len(rows)
    t = np.sort(rng.uniform(2.0, 6.0, size=(R, spr)), axis=1).astype(f32)
    s = np.zeros((R, spr), f32)
    for r, (j, k, marks) in enumerate(rows):
        s[r, k:] = f32(1e12)
        if marks in ("at_j", "both") and j < spr:
            s[r, j] = -1
        if marks in ("last", "both") and j <= spr - 1:
            s[r, spr - 1] = -1
        if j == spr and marks != "none":
            s[r, spr - 1] = -1                       # an untouched ray keeps whatever it holds
    return t, s, f32(6.5), np.array([j for j, _, _ in rows], np.int32)


def smooth_verify_rays(R, spr, seed=7):
    from . import sampling_cases as sc
    rng = np.random.default_rng([20261020, seed, spr])
    t = np.sort(rng.uniform(sc.NEAR, sc.FAR, size=(R, spr)), axis=1).astype(f32)
    s = np.stack([(sc._bumps(np.random.default_rng([20261020, seed, spr, r]), t[r]) if r % 4 != 3 else np.zeros(spr)) for r in range(R)]).astype(f32)
    jstar = rng.integers(0, spr + 1, size=R).astype(np.int32)
    for r in range(R):
        mk = (np.arange(spr) >= jstar[r]) & (rng.uniform(size=spr) < 0.2)
        s[r, mk] = -1
    return t, s, f32(sc.FAR), jstar


# ---- audit ------------------------------------------------------------------------------------------------------------------------------
def audit_model(aux, sigma, words=(0, 0, 0, 0), aux_count=None, aux_capacity=None):
    """Exact: -> (sigma afterwards, the four words), for records at DISTINCT samples.  words[0] += records, [1] += those whose value v is
    positive or NaN, [2] = max(0x7f800000 - bits(headroom)) with headroom = |v| over v <= 0, [3] = max bits(|side - v|) over the finite
    differences; sigma = 0 at every record unless v > 0."""
    a = np.asarray(aux, np.uint32).reshape(-1, 2)
    s = np.asarray(sigma, f32).reshape(-1).copy()
    n = min(len(a) if aux_count is None else aux_count, len(a) if aux_capacity is None else aux_capacity)
    w = [int(x) for x in words]
    if n == 0:
        return s, np.array(w, np.uint32)
    idx = a[:n, 0].astype(np.int64); side = np.ascontiguousarray(a[:n, 1]).view(f32)
    assert len(set(idx.tolist())) == n
    v = s[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        nonpos = v <= 0
        err = np.abs(side - v)
        finite = err <= f32(3.0e38)
        positive = v > 0
    w[0] += n
    w[1] += int(n - nonpos.sum())
    if nonpos.any():
        w[2] = max(w[2], int((0x7f800000 - np.abs(v[nonpos]).view(np.uint32).astype(np.int64)).max()))
    if finite.any():
        w[3] = max(w[3], int(err[finite].astype(f32).view(np.uint32).max()))
    s[idx[~positive]] = 0
    return s, np.array(w, np.uint32)


AUDIT_VALUES = [f32(x) for x in (-5.0, -1e-30, -0.0, 0.0, 1e-45, -1e-45, 2.5, np.nan, np.inf, -np.inf, -0.37, 3e38, -3e38)]
AUDIT_SIDES = [f32(x) for x in (-1.0, -0.26, np.nan, np.inf, -np.inf, -3e38)]


def audit_records(n, n_sigma, seed=8, values=None):
    """n records at distinct samples of a buffer of n_sigma floats: every (value, side value) combination first, then random negatives with a
    few positives; the rest of the buffer holds a sentinel that must survive."""
    rng = np.random.default_rng([20261020, seed, n])
    idx = rng.permutation(n_sigma)[:n].astype(np.uint32)
    combos = [(v, s) for v in (values or AUDIT_VALUES) for s in AUDIT_SIDES]
    v = (-rng.uniform(0.3, 40.0, size=n)).astype(f32)
    v[rng.uniform(size=n) < 0.001] = f32(0.125)
    side = (v + rng.normal(size=n).astype(f32) * f32(0.05)).astype(f32)
    for k, (a, b) in enumerate(combos[:n]):
        v[k], side[k] = a, b
    sigma = np.full(n_sigma, f32(7.5), f32)
    sigma[idx] = v
    return np.stack([idx, side.view(np.uint32)], axis=1).astype(np.uint32), sigma


# ---- the pre-filter's arithmetic, restated ----------------------------------------------------------------------------------------------
def load_net(directory):
    """{name: array} of a network directory in the reference's format (shapes.txt + little-endian f32 files; kernels are K x N)."""
    out = {}
    for line in open(os.path.join(directory, "shapes.txt")):
        name, *dims = line.split()
        out[name] = np.fromfile(os.path.join(directory, name + ".bin"), "<f4").reshape([int(d) for d in dims])
    return out


def round_bf16(x):
    """f32 -> nearest bf16 (ties to even), as f32; NaN passes."""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(f32)
    return np.where(np.isnan(x), x, r).astype(f32)


def round_f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, f32).astype(np.float16).astype(f32)       # round-to-nearest-even, overflow to inf


def encode(pts):
    """positional_encoding (src/network.rs:263-330), 10 octaves: (n, 3) f32 -> (n, 63) f32; sin / cos of the f32 product f x (exact: f is a
    power of two), evaluated in float64 and rounded once."""
    p = np.asarray(pts, f32)
    cols = [p]
    f = 1.0
    for _ in range(10):
        a = p.astype(np.float64) * f
        cols += [np.sin(a).astype(f32), np.cos(a).astype(f32)]
        f *= 2.0
    return np.concatenate(cols, axis=1)


def ray_points(origin, dirs, t):
    """(R, 3), (R, n) -> (R * n, 3) f32 points fl(o + fl(d t)) (mlp_seq_common.hip.h chunk_inputs)."""
    prod = np.asarray(dirs, f32)[:, None, :] * np.asarray(t, f32)[:, :, None]
    return (np.asarray(origin, f32)[None, None, :] + prod).astype(f32).reshape(-1, 3)


def prefilter_emulation(net, pts, kind, accumulate="f64", perm_seed=None):
    """The raw density pre-activation as the 16-bit pre-filter kernels form it (mlp_kernel_bf16v2.hip): encodings and ReLU'd activations
    rounded to 16 bits (pack2 / pack_tile), 16-bit weights, f32 biases as the accumulators' start, f32 accumulation, and the density head in f32
    from the UNROUNDED f32 accumulators of dense7 (convert_half HEAD 2).  kind: "f16" | "bf16".
    accumulate = "f64": every layer's sum in float64, rounded to f32 once (no order); "f32": f32 accumulation with the k index permuted
    (perm_seed) -- the difference between the two is what summation order alone does to the result, rounding flips downstream included."""
    rnd = round_f16 if kind == "f16" else round_bf16
    acc_t = np.float64 if accumulate == "f64" else f32
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None

    def layer(x16, name):
        w = rnd(net[name + "_kernel"]).astype(acc_t); b = net[name + "_bias"].astype(acc_t)
        x = x16.astype(acc_t)
        if rng is not None:
            p = rng.permutation(w.shape[0])
            x, w = np.ascontiguousarray(x[:, p]), np.ascontiguousarray(w[p])
        with np.errstate(invalid="ignore", over="ignore"):
            return (x @ w + b).astype(f32)

    def act(a):
        return rnd(np.where(a > 0, a, np.where(np.isnan(a), a, f32(0))).astype(f32))    # the packed ReLU keeps +inf and NaN

    e = rnd(encode(pts))
    h = act(layer(e, "dense0"))
    for i in range(1, 5):
        h = act(layer(h, f"dense{i}"))
    h = act(layer(np.concatenate([e, h], axis=1), "dense5"))
    h = act(layer(h, "dense6"))
    a7 = layer(h, "dense7")
    r7 = np.where(a7 > 0, a7, f32(0)).astype(acc_t)                                     # relu() of the f32 head: NaN -> 0
    w = net["alpha_kernel"].astype(acc_t); b = net["alpha_bias"].astype(acc_t)
    if rng is not None:
        p = rng.permutation(256)
        r7, w = np.ascontiguousarray(r7[:, p]), np.ascontiguousarray(w[p])
    with np.errstate(invalid="ignore", over="ignore"):
        return (r7 @ w + b).astype(f32).reshape(-1)


def exact_preactivation(net, pts):
    """The density pre-activation of the unrounded f32 weights, everything in float64."""
    e = encode(pts).astype(np.float64)

    def layer(x, name):
        return x @ net[name + "_kernel"].astype(np.float64) + net[name + "_bias"].astype(np.float64)

    h = np.maximum(layer(e, "dense0"), 0)
    for i in range(1, 5):
        h = np.maximum(layer(h, f"dense{i}"), 0)
    h = np.maximum(layer(np.concatenate([e, h], axis=1), "dense5"), 0)
    h = np.maximum(layer(h, "dense6"), 0)
    h = np.maximum(layer(h, "dense7"), 0)
    return layer(h, "alpha").reshape(-1)


def retirement_bounds(pre_emul, t, far, cut_T, rel=1e-3):
    """Per sample, from the emulation's transmittance at the END of each 32-sample chunk: (may be NaN, must be NaN).  A sample may be
    "not evaluated" only if T was below cut_T (1 + rel) by the end of an EARLIER chunk; it must be once T was below cut_T (1 - rel) then."""
    p = np.asarray(pre_emul, np.float64).reshape(np.asarray(t).shape)
    R, spr = p.shape
    T = np.exp(-np.cumsum(np.where(p > 0, p, 0.0) * deltas(t, far), axis=1))
    may = np.zeros((R, spr), bool); must = np.zeros((R, spr), bool)
    for c in range(1, (spr + 31) // 32):
        lo = T[:, :32 * c].min(1)                       # T only falls: its value at the end of chunk c - 1
        may[:, 32 * c:32 * (c + 1)] = (lo < cut_T * (1 + rel))[:, None]
        must[:, 32 * c:32 * (c + 1)] = (lo < cut_T * (1 - rel))[:, None]
    return may, must
