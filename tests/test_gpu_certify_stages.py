"""certify_zero's four device pieces, each through its own stage entry (nerf_stage_cert_plan / _verify / _audit, nerf_stage_prefilter: the
launches the certified render makes) against the plain float64 models of tests/helpers/certify_cases.py -- bit for bit, lists as sets --
at the shapes where each can go wrong, and one certified render restated from the stage calls down to its counters.
tests/test_certify_cases_cpu.py shows that the inputs reach the branches and that a mutant model fails these comparisons."""
import functools
import os

import numpy as np
import pytest

from conftest import ROOT, SCENE, golden
from helpers import certify_cases as cc

pytestmark = pytest.mark.gpu

f32 = np.float32
U32 = 0xFFFFFFFF
FLAG = 0x80000000


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- plan ---------------------------------------------------------------------------------------------------------------------------------
def check_plan(out, pre, m, spr, cap, acap, skip_rays=()):
    """Everything the plan stage returns against the model m.  skip_rays: guarded rays (family B), left out of every comparison.
    Where a run of rays_per_wave rays holds more than 256 picks, only the overflow invariants hold for the audits (which ones are dropped
    is not part of the contract)."""
    R = len(pre)
    rpw = out["rays_per_wave"]
    assert rpw == cc.rays_per_wave(spr)
    runs = cc.picks_per_run(m["pick"], rpw)
    staged_all = bool((runs <= cc.STAGE).all())
    assert np.all(out["guards"] == U32), "a word outside [0, capacity) was written"
    keep_ray = np.ones(R, bool); keep_ray[list(skip_rays)] = False
    kept = lambda s: {e for e in s if keep_ray[(e & 0x7FFFFFFF) // spr]}
    assert np.array_equal(out["jstar"][keep_ray], m["jstar"][keep_ray])
    nf, nb, na = out["counts"]
    back_part = m["picks_go_back"]
    if not back_part:
        assert nb == 0
    lst = out["list"]
    fits = nf + nb <= cap
    front_stored = lst[:min(nf, cap)]
    back_stored = lst[max(cap - nb, 0):] if nb else lst[:0]
    if fits:
        assert np.all(lst[nf:cap - nb] == U32) and not np.any(front_stored == U32) and not np.any(back_stored == U32)
        assert len(set(front_stored.tolist())) == nf and len(set(back_stored.tolist())) == nb            # no entry twice
    front, back = set(front_stored.tolist()) - {U32}, set(back_stored.tolist()) - {U32}
    flagged = {e & 0x7FFFFFFF for e in (front | back) if e & FLAG}
    # aux records <-> flagged entries, with the pre-activation the plan was given
    n_rec = min(na, acap)
    rec = out["aux"][:n_rec]
    assert np.all(out["aux"][n_rec:] == U32)
    rec_idx = rec[:, 0].tolist()
    assert len(set(rec_idx)) == n_rec and np.array_equal(rec[:, 1], bits(pre).reshape(-1)[rec[:, 0]])
    if fits:
        assert set(rec_idx) == flagged, "flagged list entries and aux records are not in bijection"
    else:
        assert flagged <= set(rec_idx)
    assert kept(flagged) <= kept(m["picks"]) and kept(set(rec_idx)) <= kept(m["picks"])
    # the rewritten buffer: 0, or -1 on a marked sample; an unflagged pick reads 0 like its unaudited siblings
    assert np.array_equal(bits(out["pre"])[keep_ray], bits(m["buffer"])[keep_ray])
    # uncertain samples in front of the cut: all listed (when they fit), in their part
    want_front = m["front"] if back_part else m["front"] | m["back"]
    want_back = m["back"] if back_part else set()
    got_front_unc, got_back_unc = {e for e in front if not e & FLAG}, {e for e in back if not e & FLAG}
    lost_flag = (got_front_unc | got_back_unc) & m["picks"]         # audits that found no aux record: listed without a flag (aux capacity only)
    if acap >= na:
        assert not kept(lost_flag)
    else:
        assert len(lost_flag) == na - acap if fits and staged_all else True
    if fits:
        assert kept(got_front_unc - lost_flag) == kept(want_front) and kept(got_back_unc - lost_flag) == kept(want_back)
        assert kept(lost_flag) <= (kept(back) if back_part else kept(front))
        flagged_in_front = {e & 0x7FFFFFFF for e in front if e & FLAG}
        assert not flagged_in_front if back_part else flagged_in_front == flagged
    else:
        assert kept(got_front_unc - lost_flag) <= kept(want_front | want_back) and kept(got_back_unc - lost_flag) <= kept(want_back | want_front)
    # the counters hold the NEED whatever the capacities; audits: min(picks, 256) per run of rays_per_wave rays
    if keep_ray.all():
        assert na == int(np.minimum(runs, cc.STAGE).sum())
        assert nf + nb == len(m["front"]) + len(m["back"]) + na
        if back_part:
            assert nf == len(m["front"]) and nb == len(m["back"]) + na
        if staged_all and fits and acap >= na:
            assert flagged == m["picks"]
    if fits and acap >= na:                                            # per run: exactly min(its picks, 256) audits
        per_run = np.bincount(np.array(sorted(flagged), np.int64) // spr // rpw, minlength=len(runs)) if flagged else np.zeros(len(runs), int)
        ok = np.array([keep_ray[a * rpw:(a + 1) * rpw].all() for a in range(len(runs))])
        assert np.array_equal(per_run[ok], np.minimum(runs, cc.STAGE)[ok])
    return nf, nb, na


@pytest.mark.parametrize("back_part", [True, False], ids=["back", "noback"])
@pytest.mark.parametrize("spr", cc.PLAN_SPR)
def test_plan_against_the_model(renderer, spr, back_part):
    """Families A (exact sums: j* exact, depth EQUAL to the limit is no cut), B (smooth; guarded rays left out, cap 2 %) and C (special values,
    descending t) at every n_rays; bit-exact, lists as sets."""
    skipped = total = 0
    for R in cc.PLAN_RAYS:
        salt = 0x632BE5AB * R + spr
        # A
        t, pre, far, want = cc.exact_sum_rays(R, spr)
        zt = f32(0.05) if back_part else None
        m = cc.plan_model(pre, t, far, 0.5, cc.EXACT_LIMIT, salt=salt, zero_threshold=zt)
        assert np.array_equal(m["jstar"], want)
        out = renderer.stage_cert_plan(pre, t, far, 0.5, cc.EXACT_LIMIT, audit_salt=salt, zero_threshold=zt)
        check_plan(out, pre, m, spr, R * spr, R * spr)
        # B, at both ends of the shipped margins
        t, pre, far = cc.smooth_rays(R, spr)
        for margin in (0.25, 3.0):
            zt = f32(margin) * cc.ZERO_FRAC if back_part else None
            m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=salt, zero_threshold=zt)
            guard = np.nonzero(cc.near_limit_rays(m["before"], cc.DEPTH_LIMIT))[0]
            skipped += len(guard); total += R
            out = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, audit_salt=salt, zero_threshold=zt)
            check_plan(out, pre, m, spr, R * spr, R * spr, skip_rays=guard)
        # C
        margin, ztv = f32(0.5), f32(0.05)
        t, pre, far, _ = cc.special_rays(R, spr, margin, ztv)
        zt = ztv if back_part else None
        m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, mask=7, mask_near=1, salt=salt, zero_threshold=zt)
        out = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, audit_mask=7, audit_mask_near=1, audit_salt=salt, zero_threshold=zt)
        check_plan(out, pre, m, spr, R * spr, R * spr)
    assert skipped <= cc.GUARD_CAP * total


@pytest.mark.parametrize("back_part", [True, False], ids=["back", "noback"])
@pytest.mark.parametrize("spr", [513, 800, 1070])
def test_plan_audit_stage_overflow(renderer, spr, back_part):
    """Family D: more than 256 picks per run of rays_per_wave rays.  Which audits are dropped is the kernel's business; the invariants are not:
    flagged entries <-> aux records with equal pre bits, flagged <= the model's picks, an unflagged pick is not listed and reads 0, every run
    audits exactly min(its picks, 256)."""
    margin = f32(0.5)
    rpw = cc.rays_per_wave(spr)
    R = cc.OVERFLOW_RUNS * rpw + 1
    t, pre, far = cc.overflow_rays(R, spr, margin)
    zt = f32(0.05) if back_part else None
    m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=9, zero_threshold=zt)
    assert (cc.picks_per_run(m["pick"], rpw) > cc.STAGE).any()
    out = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, audit_salt=9, zero_threshold=zt)
    nf, nb, na = check_plan(out, pre, m, spr, R * spr, R * spr)
    assert na < len(m["picks"]) and nf + nb == na                      # nothing uncertain: the list holds the audits alone
    assert not np.any(bits(out["pre"]))                                # every sample reads +0: the unflagged picks too


@pytest.mark.parametrize("back_part", [True, False], ids=["back", "noback"])
@pytest.mark.parametrize("spr,R", [(65, 33), (257, 9), (800, 8)])
def test_plan_capacities_below_need(renderer, spr, R, back_part):
    """A list shorter than the need: the counters still hold the need, what is stored is a subset of what is expected, no word outside
    [0, capacity) is written (guard words on both sides).  An aux buffer shorter than the need: the overflowed audits carry no flag."""
    margin, ztv = f32(0.5), f32(0.05)
    t, pre, far, _ = cc.special_rays(R, spr, margin, ztv)
    pre[:, : spr // 3] = np.where(np.arange(R * (spr // 3)).reshape(R, -1) % 3 == 0, f32(0.001), pre[:, : spr // 3])   # a third uncertain in front
    zt = ztv if back_part else None
    kw = dict(audit_mask=3, audit_mask_near=1, audit_salt=3, zero_threshold=zt)
    m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, mask=3, mask_near=1, salt=3, zero_threshold=zt)
    full = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, **kw)
    nf, nb, na = check_plan(full, pre, m, spr, R * spr, R * spr)
    need = nf + nb
    assert need > 40 and na > 10 and (nb > 10 or not back_part)
    for cap in (need, need - 1, max(nf, nb), max(nf, nb) // 2, 1, 0):
        out = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, list_capacity=cap, **kw)
        assert check_plan(out, pre, m, spr, cap, R * spr) == (nf, nb, na)
    for acap in (na, na - 1, na // 2, 1, 0):
        out = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, aux_capacity=acap, **kw)
        assert check_plan(out, pre, m, spr, R * spr, acap) == (nf, nb, na)
        n_flag = int(np.sum((out["list"] != U32) & (out["list"] & FLAG != 0)))
        assert n_flag == min(na, acap)


# ---- verify -------------------------------------------------------------------------------------------------------------------------------
def check_verify(out, sigma, m_sigma, m_listed, m_fb, spr, cap, start, skip_rays=()):
    R = len(sigma)
    keep_ray = np.ones(R, bool); keep_ray[list(skip_rays)] = False
    assert np.all(out["guards"] == U32)
    n_new = out["count"] - start
    stored = out["list"][start:min(out["count"], cap)] if start < cap else out["list"][:0]
    assert np.all(out["list"][:min(start, cap)] == U32) and np.all(out["list"][min(out["count"], cap):] == U32)
    got = set(stored.tolist())
    assert len(got) == len(stored) and U32 not in got
    kept = lambda s: {e for e in s if keep_ray[e // spr]}
    if keep_ray.all():
        assert n_new == len(m_listed) and out["fallback_rays"] == m_fb[0] + m_fb[1]
        assert np.array_equal(bits(out["sigma"]), bits(m_sigma))
    else:                                                               # marks are cleared either way; what differs is the list
        assert np.array_equal(bits(out["sigma"])[keep_ray], bits(m_sigma)[keep_ray])
    if out["count"] <= cap:
        assert kept(got) == kept(m_listed)
    else:
        assert kept(got) <= kept(m_listed)


@pytest.mark.parametrize("spr", [1, 2, 63, 64, 65, 192, 257, 1070])
def test_verify_against_the_model(renderer, spr):
    """One-hot rays put the exact cut at j* - 1 (marks cleared, nothing listed), at j* (every mark listed, one fall-back ray) or nowhere, for
    j* in {0, 1, 63, 64, 65, spr}; smooth rays with the near-cut guard (cap 2 %).  Counter start != 0, a list too short, n_rays not a
    multiple of 4."""
    t, s, far, js = cc.one_hot_verify_rays(spr)
    for R in sorted({len(s), len(s) - 1, max(len(s) - 2, 1), 1}):
        ms, listed, fb, near = cc.verify_model(s[:R], t[:R], far, js[:R])
        assert not near.any()
        for start, cap in ((0, R * spr), (5, R * spr), (0, len(listed) // 2), (3, 3), (7, 2), (0, 0)):
            cap = min(cap, R * spr)
            out = renderer.stage_cert_verify(s[:R], t[:R], far, js[:R], list_capacity=cap, count=start, fallback_rays=11)
            check_verify(out, s[:R], ms, listed, (11, fb), spr, cap, start)
    t, s, far, js = cc.smooth_verify_rays(130, spr)
    ms, listed, fb, near = cc.verify_model(s, t, far, js)
    assert near.mean() <= cc.GUARD_CAP
    out = renderer.stage_cert_verify(s, t, far, js)
    check_verify(out, s, ms, listed, (0, fb), spr, 130 * spr, 0, skip_rays=np.nonzero(near)[0])


# ---- audit --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 78, 1000, 200_000])
def test_audit_against_the_model(renderer, n):
    """Exact: the counts, violations (positive or NaN), the bit-encoded least headroom, the largest finite error, entries reset unless v > 0;
    n = 0 leaves the words alone; 200 000 records are more than one grid stride; the words accumulate over two calls."""
    n_sigma = max(2 * n, 16)
    aux, sigma = cc.audit_records(n, n_sigma)
    start = (3, 1, 0x7f800000 - int(f32(7.0).view(np.uint32)), int(f32(0.001).view(np.uint32)))
    for words in ((0, 0, 0, 0), start):
        want_s, want_w = cc.audit_model(aux, sigma, words)
        got_s, got_w = renderer.stage_cert_audit(aux, sigma, words)
        assert np.array_equal(got_w, want_w), (got_w, want_w)
        assert np.array_equal(bits(got_s), bits(want_s))
    if n == 0:
        assert np.array_equal(renderer.stage_cert_audit(aux, sigma, start)[1], np.array(start, np.uint32))
        return
    # two calls over the two halves accumulate to one call over the whole
    h = n // 2
    s1, w1 = renderer.stage_cert_audit(aux[:h], sigma)
    s2, w2 = renderer.stage_cert_audit(aux[h:], s1, w1)
    want_s, want_w = cc.audit_model(aux, sigma)
    assert np.array_equal(w2, want_w) and np.array_equal(bits(s2), bits(want_s))
    # a count beyond the capacity: the capacity's records, and a count below it: the count's
    for cnt, cap in ((n + 7, max(n - 1, 0)), (n // 3, n), (0, n), (n, 0)):
        want_s, want_w = cc.audit_model(aux, sigma, start, aux_count=cnt, aux_capacity=cap)
        got_s, got_w = renderer.stage_cert_audit(aux[:max(min(cnt, cap), 1)], sigma, start, aux_count=cnt, aux_capacity=cap)
        assert np.array_equal(got_w, want_w) and np.array_equal(bits(got_s), bits(want_s)), (cnt, cap)


# ---- pre-filter ---------------------------------------------------------------------------------------------------------------------------
PF_SHAPES = [(9, 1), (9, 31), (9, 32), (40, 33), (40, 64), (9, 192), (9, 200)]      # (rays, spr): chunks of 32 samples, two rays per wave, eight per workgroup
PF_SUBSETS = [1, 2, 3, 9]                                                           # (d): the first rays alone give the same bits
CUT_T = float(np.exp(-(9.6 + 0.5)))                                                 # cert_pass: the plan's depth limit + 0.5


@functools.lru_cache(maxsize=None)
def _nets(root):
    return cc.load_net(os.path.join(root, "coarse")), cc.load_net(os.path.join(root, "fine"))


@pytest.fixture(scope="module")
def rays(renderer, native, samples):
    """(R, spr) -> origin, unit directions (tests/golden/ray_dirs.npz, the rays through the object first), t from stage_stratified."""
    g = golden("ray_dirs.npz")
    order = [4, 5, 8, 9, 12, 15, 13, 14] + [0, 1, 2, 3, 6, 7, 10, 11]
    hat = g["dirhat800"][order]
    cam = native.camera_from_samples(samples, 800, 800, 64)

    @functools.lru_cache(maxsize=None)
    def make(R, spr):
        t = renderer.stage_stratified(cam, 100, 300, R, 1, spr, seed=17).reshape(R, spr)
        return np.asarray(cam.pos, f32), np.ascontiguousarray(hat[np.arange(R) % len(hat)]), t, float(cam.far)
    return make


@functools.lru_cache(maxsize=None)
def _emulated(root, which, kind, key):
    net = _nets(root)[which]
    pts = _POINTS[key]
    return (cc.prefilter_emulation(net, pts, kind, "f64"), cc.prefilter_emulation(net, pts, kind, "f32", perm_seed=which * 7 + len(pts)),
            _exact(root, which, key))


@functools.lru_cache(maxsize=None)
def _exact(root, which, key):
    return cc.exact_preactivation(_nets(root)[which], _POINTS[key])


_POINTS = {}


def _points(rays, R, spr):
    o, d, t, far = rays(R, spr)
    _POINTS.setdefault((R, spr), cc.ray_points(o, d, t))
    return (R, spr)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("which", [0, 1], ids=["coarse", "fine"])
def test_prefilter_lego(renderer, rays, which, kind):
    """The ray-sequential 16-bit pre-filter on lego, cut_T = 0 (no ray retired), every shape of PF_SHAPES:
    (a) every sample the device certifies at the margin floor (f16 0.25 / 0.5, bf16 1.0 / 3.0: nerf_internal.h) has a float64 pre-activation
        <= 0 and |device - float64| <= half the floor: the audit's own rule, on ALL certified samples instead of 1 in 128;
    (b) against the numpy emulation of the kernel's arithmetic: the CPU alone shows what summation order does (float64 layer sums against f32
        sums in a permuted k order: p99 and max of the difference over the test's points); the GPU, a third order, gets 4 x each;
    (c) no sample is NaN; (d) the first 1, 2, 3, 9 rays alone give the same bits.
    Measured over the 7 984 points of PF_SHAPES, as p99 / max of the absolute difference (coarse; fine):
      CPU, float64 sums against permuted f32 sums   f16 6.4e-3 / 0.126; 3.7e-3 / 0.089     bf16 1.5e-5 / 0.224; 3.1e-5 / 0.233
      MI355X against the float64-sum emulation      f16 7.4e-3 / 0.105; 4.1e-3 / 0.148     bf16 3.1e-5 / 0.291; 4.8e-5 / 0.847
    (the maxima are single rounding flips of an activation, carried through the layers behind it); (a): worst |device - float64| on a certified
    sample 0.015 of 0.125; 0.064 of 0.25 (f16), 0.073 of 0.5; 0.24 of 1.5 (bf16).  DESIGN 4.9 carries the same figures."""
    floor = (cc.FLOORS_F16 if kind == "f16" else cc.FLOORS_BF16)[which]
    dev, emu, emu_perm, exact = [], [], [], []
    for R, spr in PF_SHAPES:
        o, d, t, far = rays(R, spr)
        pre, bad = renderer.stage_prefilter(which, o, d, t, far, f16=kind == "f16", cut_T=0.0)
        assert bad == 0 and not np.isnan(pre).any() and np.isfinite(pre).all()                       # (c)
        for n in PF_SUBSETS:
            if n < R:
                sub, _ = renderer.stage_prefilter(which, o, d[:n], t[:n], far, f16=kind == "f16", cut_T=0.0)
                assert np.array_equal(bits(sub), bits(pre[:n])), (R, spr, n)                           # (d)
        e64, e32, ex = _emulated(SCENE, which, kind, _points(rays, R, spr))
        dev.append(pre.reshape(-1)); emu.append(e64); emu_perm.append(e32); exact.append(ex)
    dev, emu, emu_perm, exact = (np.concatenate(x).astype(np.float64) for x in (dev, emu, emu_perm, exact))
    cert = dev < -floor
    worst = np.abs(dev - exact)[cert].max()
    print(f"\nprefilter {kind} net {which}: {cert.sum()} of {len(dev)} certified at floor {floor}; max exact pre-activation on them {exact[cert].max():.4f}, "
          f"max |device - float64| on them {worst:.4f} (limit {floor / 2})")
    assert cert.sum() > 100
    assert exact[cert].max() <= 0 and worst <= floor / 2                                              # (a)
    cpu, gpu = np.abs(emu - emu_perm), np.abs(dev - emu)
    p99c, maxc, p99g, maxg = np.percentile(cpu, 99), cpu.max(), np.percentile(gpu, 99), gpu.max()
    print(f"prefilter {kind} net {which}: order spread on the CPU p99 {p99c:.3e} max {maxc:.3e}; GPU against the emulation p99 {p99g:.3e} max {maxg:.3e}")
    assert p99g <= 4 * p99c and maxg <= 4 * maxc                                                       # (b)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_prefilter_random_scene(native, rays, tmp_path_factory, kind):
    """The same four properties on random_scene(..., 11): a fog, weight statistics unlike lego's (no floors shipped for it: (a) is held at lego's)."""
    root = str(_random_root(tmp_path_factory))
    with native.Renderer(0) as r:
        r.load_scene(root)
        for which in (0, 1):
            floor = (cc.FLOORS_F16 if kind == "f16" else cc.FLOORS_BF16)[which]
            dev, emu, emu_perm, exact = [], [], [], []
            for R, spr in ((9, 33), (9, 64)):
                o, d, t, far = rays(R, spr)
                pre, bad = r.stage_prefilter(which, o, d, t, far, f16=kind == "f16", cut_T=0.0)
                assert bad == 0 and np.isfinite(pre).all()
                sub, _ = r.stage_prefilter(which, o, d[:3], t[:3], far, f16=kind == "f16", cut_T=0.0)
                assert np.array_equal(bits(sub), bits(pre[:3]))
                e64, e32, ex = _emulated(root, which, kind, _points(rays, R, spr))
                dev.append(pre.reshape(-1)); emu.append(e64); emu_perm.append(e32); exact.append(ex)
            dev, emu, emu_perm, exact = (np.concatenate(x).astype(np.float64) for x in (dev, emu, emu_perm, exact))
            cert = dev < -floor
            if cert.any():
                assert exact[cert].max() <= 0 and np.abs(dev - exact)[cert].max() <= floor / 2
            cpu, gpu = np.abs(emu - emu_perm), np.abs(dev - emu)
            print(f"\nprefilter {kind} random net {which}: {cert.sum()} certified; CPU p99 {np.percentile(cpu, 99):.3e} max {cpu.max():.3e}; "
                  f"GPU p99 {np.percentile(gpu, 99):.3e} max {gpu.max():.3e}")
            assert np.percentile(gpu, 99) <= 4 * np.percentile(cpu, 99) and gpu.max() <= 4 * cpu.max()


_RANDOM = {}


def _random_root(tmp_path_factory):
    if "root" not in _RANDOM:
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from scene_utils import random_scene
        _RANDOM["root"] = random_scene(tmp_path_factory.mktemp("certify_stages") / "scene", 11)
    return _RANDOM["root"]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_prefilter_retires_rays_by_chunk(renderer, rays, kind):
    """cut_T = exp(-(9.6 + 0.5)): a ray is retired after the 32-sample chunk in which its transmittance fell below cut_T.  From the emulation's
    transmittance: a sample reads "not evaluated" only if T was below cut_T (1 + 1e-3) by the end of an earlier chunk, and every sample of a
    later chunk does once it was below cut_T (1 - 1e-3); whatever was evaluated carries the bits of the run without a cut."""
    retired = 0
    for which in (0, 1):
        for R, spr in ((9, 192), (9, 200), (40, 64), (9, 32)):
            o, d, t, far = rays(R, spr)
            full, _ = renderer.stage_prefilter(which, o, d, t, far, f16=kind == "f16", cut_T=0.0)
            pre, bad = renderer.stage_prefilter(which, o, d, t, far, f16=kind == "f16", cut_T=CUT_T)
            nan = np.isnan(pre)
            assert bad == 0 and np.all(bits(pre)[nan] == U32) and np.array_equal(bits(pre)[~nan], bits(full)[~nan])
            may, must = cc.retirement_bounds(_emulated(SCENE, which, kind, _points(rays, R, spr))[0], t, far, CUT_T)
            assert not (nan & ~may).any() and not (must & ~nan).any(), (which, R, spr)
            retired += int(nan.sum())
    print(f"\nprefilter {kind}: {retired} samples behind a retirement")
    assert retired > 100


def test_prefilter_f16_leaves_its_range(native, rays, tmp_path):
    """The lego network scaled as in test_gpu_certify.py's test_network_beyond_the_f16_range_...: dense0 x 2000, dense1 x 50 -- the f16
    pre-filter's pre-activations come out non-finite and the tiles are counted; the bf16 form stays finite and counts nothing."""
    import shutil
    root = tmp_path / "big"
    shutil.copytree(SCENE, root)
    for which in ("coarse", "fine"):
        for name, k in (("dense0_kernel", 2000.0), ("dense0_bias", 2000.0), ("dense1_kernel", 50.0), ("dense1_bias", 50.0)):
            f = root / which / f"{name}.bin"
            (np.fromfile(f, "<f4") * f32(k)).astype("<f4").tofile(f)
    o, d, t, far = rays(9, 64)
    with native.Renderer(0) as r:
        r.load_scene(str(root))
        for which in (0, 1):
            pre, bad = r.stage_prefilter(which, o, d, t, far, f16=True)
            assert bad > 0 and not np.isfinite(pre).all()
            pre, bad = r.stage_prefilter(which, o, d, t, far, f16=False)
            assert bad == 0 and np.isfinite(pre).all()


# ---- one certified render, restated from the stage calls ------------------------------------------------------------------------------------
def test_a_certified_render_restated_to_its_counters(renderer, native, samples):
    """An 800 x 800 lego crop of 40 x 24 pixels, 64 + 128 samples, certify_zero, restated per network as: pre-filter stage -> plan stage ->
    density_batch at the listed points into the plan's buffer -> audit stage -> verify stage -> density_batch at list 2.  Mirrored from
    nerf_internal.h / nerf_render.cpp cert_pass: depth limit 9.6, audit masks 127 / 15, zero fraction 0.1, pre-filter cut exp(-(9.6 + 0.5)),
    salt = (seed x 0x9E3779B97F4A7C15 >> 32) + 0x632BE5AB x pass + network; the margins come from the render's stats.  The counters as
    nerf_render.cpp defines them: n_exec_*_trunk = list 1 (front + back part, audited certificates included) + list 2 of that network;
    n_certify_audited = the audit's count over both networks; n_certify_fallback_rays = rays of both networks whose cut was not confirmed.
    The restated densities equal density_batch wherever the composited weight is non-zero."""
    from helpers import render_restatement as rr
    nc, nf, seed, crop = 64, 128, 3, (380, 388, 40, 24)
    cam = native.camera_from_samples(samples, 800, 800, nc)
    img, st = native.render_image(renderer.coarse, renderer.fine, cam, nf, seed=seed, crop=crop, certify_zero=True, return_stats=True)
    assert st.n_certify_retries == 0 and st.n_passes == 1 and st.n_certify_violations == 0
    be = rr.GpuBackend(native, renderer)
    x0, y0, w, h = crop
    W, origin, _, far = be.geometry(cam)
    dirs = be.ray_dirs(cam, x0, y0, w, h)
    pix = rr.pixel_indices(W, x0, y0, w, h)
    R = len(dirs)
    f16 = tuple(st.certify_margin) == cc.FLOORS_F16                     # lego fits the f16 range: the pre-filter runs in f16 at those floors
    assert f16
    audit_words = [None, None]
    listed = [0, 0]
    fallback = 0

    def certified_pass(which, t):
        nonlocal fallback
        spr = t.shape[1]
        margin = f32(st.certify_margin[which])
        pts = rr.ray_points(origin, dirs, t)                           # (3, R spr)
        pre, bad = renderer.stage_prefilter(which, origin, dirs, t, far, f16=True, cut_T=CUT_T)
        assert bad == 0
        salt = ((seed * 0x9E3779B97F4A7C15 & (2 ** 64 - 1)) >> 32) + 0x632BE5AB * 0 + which & U32
        colour = which == 1                                             # the colour-producing pass has the back part (cert_zero_tiles)
        plan = renderer.stage_cert_plan(pre, t, far, margin, cc.DEPTH_LIMIT, cc.MASK, cc.MASK_NEAR, salt,
                                        zero_threshold=margin * cc.ZERO_FRAC if colour else None)
        nfr, nb, na = plan["counts"]
        entries = np.concatenate([plan["list"][:nfr], plan["list"][R * spr - nb:]]) if nb else plan["list"][:nfr]
        idx = (entries & 0x7FFFFFFF).astype(np.int64)
        net = renderer.fine if which else renderer.coarse
        sigma = plan["pre"].reshape(-1).copy()
        exact = net.density(np.ascontiguousarray(pts[:, idx]))
        sigma[idx] = exact
        # an audited certificate leaves the exact kernel as its RAW pre-activation: non-positive unless the certificate is wrong, and then
        # relu = 0 = what density() returned; the audit needs the raw value only for its headroom / error words, which this test does not
        # restate (no public call returns a raw exact pre-activation) -- its COUNT is the number of records
        aud_s, words = renderer.stage_cert_audit(plan["aux"][:na], sigma)
        assert int(words[0]) == na and int(words[1]) == 0
        ver = renderer.stage_cert_verify(aud_s.reshape(R, spr), t, far, plan["jstar"])
        sigma2 = ver["sigma"].reshape(-1)
        l2 = ver["list"][:ver["count"]].astype(np.int64)
        sigma2[l2] = net.density(np.ascontiguousarray(pts[:, l2]))
        listed[which] = nfr + nb + ver["count"]
        audit_words[which] = words
        fallback += ver["fallback_rays"]
        return sigma2.reshape(R, spr), pts

    t_c = be.stratified(cam, x0, y0, w, h, nc, seed)
    sigma_c, pts_c = certified_pass(0, t_c)
    t_f = be.resample(t_c, sigma_c, nf, far, seed, pix)
    sigma_f, pts_f = certified_pass(1, t_f)
    print(f"\nrestated: lists {listed} of {R * nc} / {R * (nc + nf)}, audited {[int(a[0]) for a in audit_words]}, fall-back rays {fallback}; "
          f"render: {st.n_exec_coarse_trunk} / {st.n_exec_fine_trunk}, {st.n_certify_audited}, {st.n_certify_fallback_rays}")
    assert listed[0] == st.n_exec_coarse_trunk and listed[1] == st.n_exec_fine_trunk
    assert int(audit_words[0][0]) + int(audit_words[1][0]) == st.n_certify_audited
    assert fallback == st.n_certify_fallback_rays
    # the certified densities are the plain ones wherever a sample's weight is non-zero -- and so the frame is the render's frame
    plain_f = renderer.fine.density(pts_f).reshape(R, -1)
    _, w_plain = be.integrate(np.zeros((R, nc + nf, 3), f32), plain_f, t_f, far)
    live = w_plain != 0
    assert live.sum() > 1000 and np.array_equal(bits(sigma_f)[live], bits(plain_f)[live])
    plain_c = renderer.coarse.density(pts_c).reshape(R, -1)
    _, wc = be.integrate(np.zeros((R, nc, 3), f32), plain_c, t_c, far)
    assert np.array_equal(bits(sigma_c)[wc != 0], bits(plain_c)[wc != 0])
    _, w_cert = be.integrate(np.zeros((R, nc + nf, 3), f32), sigma_f, t_f, far)
    assert np.array_equal(bits(w_cert), bits(w_plain))
