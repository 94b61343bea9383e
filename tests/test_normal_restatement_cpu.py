"""tests/helpers/normal_restatement.py checked on the CPU, before the GPU tests of the normals lean on it (no GPU):

  * on the analytic field sigma = relu(k (R - |p|)) the restated gradient is -k p / |p| inside the ball and 0 outside, and the normal of
    rays aimed at the ball's centre is the radial direction -d, within a bound derived below from h and the f32 rounding of sigma;
  * the edge cases of the contract: a zero denominator gives a zero component (not 0 / 0), a ray without a live sample gives (0, 0, 0),
    a NaN sigma+ gives a zero normal through the "not finite" rule;
  * on a lego window (oracle networks, 20 + 50 samples, h = 1e-3) at least 90 % of the rays with opacity > 0.5 carry a normal that faces
    the camera (n . d < 0).  Obtained: 107 of 112 = 95.5 %;
  * three mutants of the restatement each change the normals of those rays: p+ and p- swapped (every ray: the normal flips), the sum run
    in descending order (obtained: 102 of 112 rays, 91 %, change in at least one bit), "live" taken as w >= 0 while a NaN sigma+ sits on the
    samples of weight 0 (every ray: the normal becomes zero)."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENE  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import normal_restatement as NR  # noqa: E402
import ray_batch_restatement as RB  # noqa: E402
import render_restatement as RR  # noqa: E402

# the window both this file and tests/test_gpu_normals.py use for the oracle-backed normals
LEGO_NORMALS = dict(W=96, crop=(19, 65, 12, 10), nc=20, nf=50, seed=7, h=1e-3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_density(net):
    """points (3, B) -> sigma (B,) of an oracle network (the density does not depend on the direction: any unit vector serves)."""
    def f(pts):
        pts = np.ascontiguousarray(pts, np.float32)
        return net.forward_batch(pts, np.tile(np.float32([0.0, 0.0, 1.0]), (pts.shape[1], 1)))[1]
    return f


# ---- analytic field ---------------------------------------------------------------------------------------------------------------
K, RADIUS = 40.0, 1.0


def ball(pts):
    """relu(K (RADIUS - |p|)) evaluated in float64 and rounded ONCE to float32: |error| <= half an ulp, <= 2^-24 K RADIUS."""
    p = np.asarray(pts, np.float64)
    return np.maximum(K * (RADIUS - np.sqrt((p * p).sum(axis=0))), 0.0).astype(np.float32)


def gradient_bound(h, r_min):
    """|restated g_a - exact g_a| for a point whose six stencil points lie inside the ball at |p| >= r_min.
    Truncation: the central difference of f over the step actually taken (den / 2, which is h up to ulp(p) / h < 1e-4 here) errs by
    h^2 / 6 |f'''|, and every third partial derivative of |p| is at most 3 / |p|^2: K h^2 / (2 r_min^2), times 1.01 for the step.
    Rounding: each sigma carries <= 2^-24 K RADIUS, the subtraction and the division <= 2^-23 |g| each (|g| <= K); den is exact
    (p+ and p- lie within a factor 2 of each other, or are both tiny)."""
    return 1.01 * K * h * h / (2.0 * r_min * r_min) + 2.0 * 2.0 ** -24 * K * RADIUS / (2.0 * h * 0.99) + 2.0 * 2.0 ** -23 * K


@pytest.mark.parametrize("h", [1e-2, 1e-3])
def test_gradient_of_the_ball_is_radial(h):
    rng = np.random.default_rng(5)
    u = rng.normal(size=(3, 400)); u /= np.sqrt((u * u).sum(axis=0))
    r_in = rng.uniform(0.3 + 2 * h, RADIUS - 0.05, 200)
    r_out = rng.uniform(RADIUS + 0.05, 2.0, 200)
    pts = (u * np.concatenate([r_in, r_out])).astype(np.float32)
    g = NR.gradient(ball, pts, h)
    p64 = pts.astype(np.float64)
    exact = -K * p64 / np.sqrt((p64 * p64).sum(axis=0))
    bound = gradient_bound(h, 0.3)
    err = np.abs(g[:, :200] - exact[:, :200]).max()
    print(f"\nh = {h}: largest |g - exact| inside {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert (g[:, 200:] == 0).all()                                   # sigma is exactly 0 at all six stencil points
    assert np.abs(g[:, :200]).max() > 0.5 * K / np.sqrt(3.0)         # and the inside is not trivially zero


def _ball_rays(h):
    """Rays aimed at the ball's centre from five origins; samples placed by hand so that no stencil crosses the kink at |p| = RADIUS:
    three outside the ball, then from RADIUS - 0.05 inwards down to 0.35 (the T < 1e-4 cut falls near |p| = 0.32 for K = 40)."""
    import oracle_py as O
    radii = np.concatenate([[1.5, 1.3, 1.1], np.arange(RADIUS - 0.05, 0.34, -0.05)])
    origins = np.float32([[0, 0, 4], [3, 0, 0], [2, 2, 1], [-1, 2.5, -2], [0.5, -3, 1.5]])
    dirs = np.stack([O.normalize((-o).astype(np.float32)) for o in origins])
    t = np.stack([(np.sqrt((o.astype(np.float64) ** 2).sum()) - radii).astype(np.float32) for o in origins])
    w = []
    for r in range(len(origins)):
        sigma = ball(NR.ray_points(origins[r], dirs[r], t[r]))
        w.append(O.compute_weights(sigma, t[r], float(t[r][-1]) + 0.05))
    return origins, dirs, t, np.stack(w)


@pytest.mark.parametrize("h", [1e-2, 1e-3])
def test_ray_normal_of_the_ball_is_radial(oracle, h):
    origins, dirs, t, w = _ball_rays(h)
    assert ((w > 0).sum(axis=1) >= 5).all() and (w[:, :3] == 0).all()
    n = NR.ray_normals(ball, origins, dirs, t, w, h)
    # every live g is within gradient_bound (per component) of K d, so G / sum(w) is within it of K d (plus the sum's own rounding,
    # <= 14 terms x 2^-23 relative); normalising a vector K d + e, |e| <= sqrt(3) bound, moves the unit vector by at most 2 |e| / K
    bound = 2.0 * np.sqrt(3.0) * (gradient_bound(h, 0.3) / K + 14 * 2.0 ** -23) + 2.0 ** -22
    err = np.abs(n + dirs).max()
    print(f"\nh = {h}: largest |n - (-d)| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert np.allclose((n.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_zero_denominator_gives_a_zero_component():
    p = np.float32([[100.0], [0.5], [-100.0]])
    h = 1e-7                                                         # below half an ulp of 100 (3.8e-6), above half an ulp of 0.5 (3e-8)
    st = NR.stencil(p, h)
    assert st[0, 0] == st[0, 1] == np.float32(100.0) and st[2, 4] == st[2, 5] and st[1, 2] != st[1, 3]
    g = NR.gradient(lambda q: np.maximum(np.asarray(q, np.float32)[1], 0).astype(np.float32), p, h)
    assert _bits(g[0])[0] == 0 and _bits(g[2])[0] == 0               # +0, not the NaN of 0 / 0
    assert g[1, 0] == 1.0
    # a non-finite sigma does not get past a zero denominator either
    g = NR.gradient(lambda q: np.full(np.asarray(q).shape[1], np.nan, np.float32), p, h)
    assert _bits(g[0])[0] == 0 and _bits(g[2])[0] == 0 and np.isnan(g[1, 0])


def test_ray_without_a_live_sample_has_a_zero_normal(oracle):
    origins, dirs, t, w = _ball_rays(1e-3)
    w = w.copy(); w[1] = 0.0; w[3, 2] = np.nan; w[3, 3:] = 0.0       # a NaN weight is not live
    n = NR.ray_normals(ball, origins, dirs, t, w, 1e-3)
    assert (_bits(n[1]) == 0).all() and (_bits(n[3]) == 0).all() and (np.abs(n[[0, 2, 4]]).sum(axis=1) > 0.9).all()
    assert (NR.ray_normals(ball, origins, dirs, t, np.zeros_like(w), 1e-3) == 0).all()


def test_a_nan_sigma_plus_gives_a_zero_normal(oracle):
    origins, dirs, t, w = _ball_rays(1e-3)
    first = np.cumsum((w > 0).sum(axis=1))[1]                        # list position of ray 2's first live sample

    def plant(sigma, w_listed):
        sigma = sigma.copy(); sigma[first] = np.nan                  # block 0: sigma at p + h e_x
        return sigma
    n, ref = NR.ray_normals(ball, origins, dirs, t, w, 1e-3, corrupt=plant), NR.ray_normals(ball, origins, dirs, t, w, 1e-3)
    assert (_bits(n[2]) == 0).all()
    assert np.array_equal(_bits(n[[0, 1, 3, 4]]), _bits(ref[[0, 1, 3, 4]]))       # no other ray is touched


# ---- the lego window ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lego(oracle, oracle_nets, samples):
    P = LEGO_NORMALS
    be = RR.OracleBackend(oracle, *oracle_nets)
    cam = oracle.camera_from_samples(samples, P["W"], P["W"])
    origin, dirs, near, far, pix = RB.camera_batch(be, cam, P["crop"])
    rs = RB.restate_rays(be, origin, dirs, near, far, None, pix, P["nc"], P["nf"], P["seed"], False, "f32")
    density = oracle_density(oracle_nets[1])
    args = (density, origin, rs["dirs"], rs["t_fine"], rs["w_fine"], P["h"])
    return dict(rs=rs, args=args, normals=NR.ray_normals(*args), hit=rs["opacity"] > 0.5)


def test_lego_normals_face_the_camera(lego):
    """Obtained on the oracle's networks: 112 of the 120 rays have opacity > 0.5; 107 of them (95.5 %) face the camera."""
    n, d, hit = lego["normals"], lego["rs"]["dirs"], lego["hit"]
    assert hit.sum() >= 100 and (~hit).any()
    assert np.allclose((n[hit].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-6)
    facing = (n * d).sum(axis=1) < 0
    share = float(facing[hit].mean())
    print(f"\nlego {LEGO_NORMALS['crop']}: {int(hit.sum())} rays with opacity > 0.5, {int(facing[hit].sum())} face the camera ({share:.3f})")
    assert share >= 0.90, share
    empty = lego["rs"]["opacity"] == 0                                # a ray that met nothing has no live sample
    assert (n[empty] == 0).all()


def _changed(a, b, hit):
    return float((_bits(a[hit]) != _bits(b[hit])).any(axis=1).mean())


def test_mutant_swapped_stencil_flips_every_normal(lego):
    m = NR.ray_normals(*lego["args"], swap=True)
    share = _changed(m, lego["normals"], lego["hit"])
    print(f"\nswapped p+ / p-: {share:.3f} of the rays change")
    assert share == 1.0
    assert np.array_equal(m[lego["hit"]], -lego["normals"][lego["hit"]])


def test_mutant_descending_sum_changes_bits(lego):
    """Obtained: 102 of the 112 rays (91 %) differ in at least one bit.  A ray keeps its bits only if no rounding of its ~20 live terms depends on
    the order; half of the rays changing is the least a bit-for-bit comparison needs to tell the two orders apart on this window."""
    m = NR.ray_normals(*lego["args"], descending=True)
    share = _changed(m, lego["normals"], lego["hit"])
    print(f"\ndescending accumulation: {share:.3f} of the rays change")
    assert share >= 0.5, share
    assert np.abs(m - lego["normals"]).max() < 1e-4                   # a rounding-level mutant: only bit equality sees it


def test_mutant_live_as_w_ge_0_lets_a_dead_sample_in(lego):
    """A NaN sigma+ planted on the listed samples of weight 0: the contract lists none (nothing changes); 'live iff w >= 0' lists them all
    and every ray that has one -- all of them: the samples behind the T cut and in empty space -- loses its normal."""
    def plant(sigma, w_listed):
        sigma = sigma.copy(); sigma[:len(w_listed)][w_listed == 0] = np.nan
        return sigma
    kept = NR.ray_normals(*lego["args"], corrupt=plant)
    assert np.array_equal(_bits(kept), _bits(lego["normals"]))
    m = NR.ray_normals(*lego["args"], live_ge=True, corrupt=plant)
    share = _changed(m, lego["normals"], lego["hit"])
    print(f"\nlive as w >= 0 with a NaN on dead samples: {share:.3f} of the rays change")
    assert share == 1.0 and (m[lego["hit"]] == 0).all()
    # without the NaN the two predicates agree: a weight of 0 multiplies whatever gradient there is
    assert np.array_equal(_bits(NR.ray_normals(*lego["args"], live_ge=True)), _bits(lego["normals"]))
