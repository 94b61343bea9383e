"""tests/helpers/certify_cases.py is fit for purpose (CPU only): the guard caps hold for the chosen seeds, family A's sums are exact in any
order, every special value lands in the class it is meant to hit, the audit hash selects the documented share -- and each mutant model
(a pick fraction of 1/32 in the near band, a cut one sample early, a near band with >=, a verify that looks one sample less) loses against
the real one on these very inputs, so the GPU comparisons of tests/test_gpu_certify_stages.py would see a kernel that made that mistake."""
import numpy as np
import pytest

from helpers import certify_cases as cc

f32 = np.float32


@pytest.mark.parametrize("spr", cc.PLAN_SPR)
def test_family_a_sums_are_exact_in_any_order_and_cut_where_planned(spr):
    R = 33
    t, pre, far, want = cc.exact_sum_rays(R, spr)
    d = (np.concatenate([t[:, 1:], np.full((R, 1), far, f32)], axis=1) - t).astype(f32)
    assert np.all(d == f32(2.0 ** -6)) and np.all(pre * 16 == np.round(pre * 16)) and np.abs(pre).max() <= 32
    od = (np.maximum(pre, 0) * d).astype(f32)
    rng = np.random.default_rng(5)
    for r in range(R):
        exact = float(od[r].astype(np.float64).sum())
        for _ in range(3):                                                   # f32 running sums in permuted orders: all the same number
            acc = f32(0)
            for v in od[r][rng.permutation(spr)]:
                acc = f32(acc + v)
            assert float(acc) == exact
    m = cc.plan_model(pre, t, far, 0.5, cc.EXACT_LIMIT)
    assert np.array_equal(m["jstar"], want)
    cut = want < spr
    at = np.clip(want - 1, 0, spr - 1)
    before = m["before"][np.arange(R), at]
    assert np.all(before[cut & (want >= 2)] == float(cc.EXACT_LIMIT))        # the sample before the cut stands AT the limit: strict >
    assert set(np.unique(want)) == set(c for c in cc.EXACT_CUTS + (spr - 1,) if 0 < c < spr) | {spr}
    early = cc.plan_model(pre, t, far, 0.5, cc.EXACT_LIMIT, cut_early=1)     # mutant: every cut one sample early
    assert (early["jstar"] != want).sum() == cut.sum()


def test_family_b_guard_stays_under_its_cap():
    for spr in cc.PLAN_SPR:
        t, pre, far = cc.smooth_rays(65, spr)
        for margin in (0.25, 3.0):
            m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT)
            assert cc.near_limit_rays(m["before"], cc.DEPTH_LIMIT).mean() <= cc.GUARD_CAP, (spr, margin)
    # the family is not trivial: cuts, no cuts, all three classes
    t, pre, far = cc.smooth_rays(65, 192)
    m = cc.plan_model(pre, t, far, 1.0, cc.DEPTH_LIMIT, zero_threshold=0.1)
    assert 5 < (m["jstar"] < 192).sum() < 60 and len(m["front"]) > 100 and len(m["back"]) > 100 and len(m["picks"]) > 20 and m["marked"].sum() > 100


def test_special_values_land_in_their_classes():
    margin, zt = f32(0.5), f32(0.05)
    vals = cc.special_values(margin, zt)
    assert set(vals) == set(cc.SPECIAL_CLASS)
    assert vals["not_evaluated"].view(np.uint32) == 0xFFFFFFFF and np.isnan(vals["not_evaluated"])
    for name, v in vals.items():
        pre = np.array([[v, f32(-0.75)]], f32); t = np.array([[2.0, 3.0]], f32)
        m = cc.plan_model(pre, t, 4.0, margin, 9.6, mask=0, mask_near=0, zero_threshold=zt)
        cert, near, back = cc.SPECIAL_CLASS[name]
        assert bool(m["uncertain"][0, 0]) == (not cert), name
        if cert:
            assert bool(m["near"][0, 0]) == near and 0 in m["picks"], name
            # the two masks tell the bands apart: with only the near mask open, a far certificate is not picked
            only_near = cc.plan_model(pre, t, 4.0, margin, 9.6, mask=0xFFFFFFFF, mask_near=0, salt=1, zero_threshold=zt)
            assert (0 in only_near["picks"]) == near and not cc.audit_pick(0, 1, 0xFFFFFFFF), name
        else:
            assert (0 in m["back"]) == back and (0 in m["front"]) == (not back), name
    # in a family-C ray every name is present and, with a cut in the middle, on both sides of it across the rays
    t, pre, far, where = cc.special_rays(65, 192, margin, zt)
    m = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, zero_threshold=zt)
    assert set(where) == set(vals) and (np.diff(t, axis=1) < 0).any()
    for name, places in where.items():
        sides = {bool(i < m["jstar"][r]) for r, i in places if pre[r, i].view(np.uint32) == vals[name].view(np.uint32)}
        assert sides == ({True, False} if name != "+inf" else sides), name
    assert (m["jstar"] < 192).sum() > 20 and (m["jstar"] == 192).sum() > 5


def test_mutants_lose_on_these_inputs():
    margin, zt = f32(0.5), f32(0.05)
    for spr in (65, 257):
        t, pre, far, _ = cc.special_rays(33, spr, margin, zt)
        real = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=77, zero_threshold=zt)
        sparse = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=77, zero_threshold=zt, pick_shift=1)     # 1/32 and 1/256
        assert sparse["picks"] < real["picks"] and len(real["picks"]) - len(sparse["picks"]) > 10
    # the near band with >=: only a value AT -2 margin tells them apart, in front of the cut, at an index the near mask picks and the far one does not
    t, pre, far = cc.overflow_rays(4, 513, margin)
    pre[:] = f32(-2) * margin
    real = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=5)
    incl = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, salt=5, near_inclusive=True)
    assert len(incl["picks"] - real["picks"]) > 50 and not real["near"].any()
    t, pre, far, where = cc.special_rays(65, 192, margin, zt)
    r_i = [(r, i) for r, i in where["-2margin"] if pre[r, i] == f32(-2) * margin]
    real = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, mask=0xFFFFFFFF, mask_near=0, zero_threshold=zt)
    incl = cc.plan_model(pre, t, far, margin, cc.DEPTH_LIMIT, mask=0xFFFFFFFF, mask_near=0, zero_threshold=zt, near_inclusive=True)
    assert len(incl["picks"] - real["picks"]) >= 5 and len(r_i) >= 30
    # verify: one sample less in the prefix turns "cut at j* - 1" into a fall-back ray
    for spr in (65, 192):
        t, s, far, js = cc.one_hot_verify_rays(spr)
        real = cc.verify_model(s, t, far, js)
        short = cc.verify_model(s, t, far, js, cut_early=1)
        assert short[2] > real[2] and real[1] < short[1]
        assert real[2] >= 3 and len(real[1]) >= 4 and not real[3].any()


def test_verify_guard_stays_under_its_cap_and_cases_cover_the_outcomes():
    for spr in (1, 2, 63, 64, 65, 192, 257):
        t, s, far, js = cc.smooth_verify_rays(130, spr)
        out, listed, fb, near = cc.verify_model(s, t, far, js)
        assert near.mean() <= cc.GUARD_CAP, spr
        assert not (out == -1)[np.arange(spr)[None, :] >= js[:, None]].any()
        if spr >= 63:
            assert fb > 5 and len(listed) > 20 and (js < spr).sum() - fb > 5
    t, s, far, js = cc.one_hot_verify_rays(192)
    assert set(js) == {0, 1, 63, 64, 65, 192}


def test_hash_selects_its_share():
    idx = np.arange(100_000) + 12_345
    for mask in (15, 127):
        for salt in (0, 0x632BE5AB, 0xDEADBEEF):
            share = cc.audit_pick(idx, salt, mask).mean() * (mask + 1)
            assert 0.9 <= share <= 1.1, (mask, salt, share)


def test_overflow_family_overflows_from_513_samples():
    for spr in (513, 800, 1070):
        rpw = cc.rays_per_wave(spr)
        t, pre, far = cc.overflow_rays(cc.OVERFLOW_RUNS * rpw + 1, spr, 0.5)
        m = cc.plan_model(pre, t, far, 0.5, cc.DEPTH_LIMIT)
        runs = cc.picks_per_run(m["pick"], rpw)
        assert not m["uncertain"].any() and m["near"].all() and (m["jstar"] == spr).all()
        assert (runs > cc.STAGE).any() and (spr == 513 or (runs[:-1] > cc.STAGE).all()), (spr, runs)   # 513: 256.5 picks per run on average
    assert [cc.rays_per_wave(s) for s in (1, 192, 768, 800, 1070)] == [8, 8, 8, 7, 5]
    assert cc.picks_per_run(cc.plan_model(*cc.overflow_rays(8, 257, 0.5)[:2], 6.1, 0.5, cc.DEPTH_LIMIT)["pick"], 8).max() < cc.STAGE


def test_audit_model_on_hand_written_records():
    aux = np.array([[2, f32(-1.0).view(np.uint32)], [0, f32(-0.5).view(np.uint32)], [5, f32(-2.0).view(np.uint32)], [4, f32(-1.0).view(np.uint32)]], np.uint32)
    sigma = np.array([-0.25, 9.0, -1.5, 9.0, 0.5, np.nan], f32)
    out, w = cc.audit_model(aux, sigma)
    assert list(w[:2]) == [4, 2]                                             # 0.5 and NaN are violations
    assert int(w[2]) == 0x7f800000 - int(f32(0.25).view(np.uint32))           # least headroom: 0.25
    assert int(w[3]) == int(f32(1.5).view(np.uint32))                         # largest finite error: |-1.0 - 0.5|
    assert np.array_equal(out, np.array([0, 9.0, 0, 9.0, 0.5, 0], f32))
    out2, w2 = cc.audit_model(aux[:1], out, words=w)                          # accumulation: sample 2 now reads 0 -> headroom 0
    assert list(w2[:2]) == [5, 2] and int(w2[2]) == 0x7f800000 and int(w2[3]) == int(w[3])
    assert np.array_equal(cc.audit_model(aux, sigma, aux_count=9, aux_capacity=2)[1][:2], [2, 0])
    # both zeros are a headroom of +0
    for z in (f32(0.0), f32(-0.0)):
        assert int(cc.audit_model(aux[:1], np.array([0, 0, z], f32))[1][2]) == 0x7f800000


def test_rounding_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 65520.0, 1e-8, np.inf], f32)
    assert np.array_equal(cc.round_bf16(x)[:3], np.array([1.0, 1.0, 1.015625], f32))      # ties to even: 1 + 2^-8 -> 1, 1 + 3 x 2^-8 -> 1 + 2^-6
    assert np.isinf(cc.round_f16(x)[4]) and cc.round_f16(x)[5] == 0 and cc.round_f16(f32(1.0 + 2.0 ** -11)) == 1
    assert np.isnan(cc.round_bf16(np.array([np.nan], f32))[0]) and np.isinf(cc.round_bf16(x)[6])
    assert np.all(cc.round_bf16(x).view(np.uint32) & 0xFFFF == 0)
