"""Density gradients and per-ray normals restated in NumPy float32 (the contract: include/nerf_mi355x.h, "surface normals").

`density` is any callable from points (3, B) float32 SoA to sigma (B,): the CPU oracle's network, Network.density of a context, or an
analytic field -- the same code runs on all three.  Nothing here shares code with the kernels; the sums are Python loops over np.float32
scalars, so that every operation is rounded once, in the order the contract states.  The positions, t and w of a batch come from
ray_batch_restatement.restate_rays / render_restatement.restate (dirs, t_fine, w_fine) as they are."""
import numpy as np

F = np.float32


def stencil(points, h):
    """(3, B) -> (3, 6 B): block k = 2 * axis + (0: plus, 1: minus) holds the points with coordinate `axis` replaced by fl(p + h) / fl(p - h)."""
    p = np.ascontiguousarray(points, np.float32)
    h = F(h)
    blocks = []
    for axis in range(3):
        for moved in ((p[axis] + h).astype(np.float32), (p[axis] - h).astype(np.float32)):
            q = p.copy()
            q[axis] = moved
            blocks.append(q)
    return np.ascontiguousarray(np.hstack(blocks))


def _differences(st, sigma, B):
    """g (3, B) from the stencil points and their sigma: fl(fl(s+ - s-) / fl(p+ - p-)), 0 where the denominator is 0."""
    g = np.zeros((3, B), np.float32)
    for axis in range(3):
        plus, minus = slice(2 * axis * B, (2 * axis + 1) * B), slice((2 * axis + 1) * B, (2 * axis + 2) * B)
        den = (st[axis, plus] - st[axis, minus]).astype(np.float32)
        num = (sigma[plus] - sigma[minus]).astype(np.float32)
        ok = den != 0
        with np.errstate(all="ignore"):
            g[axis, ok] = (num[ok] / den[ok]).astype(np.float32)
    return g


def gradient(density, points, h, swap=False):
    """The gradient of sigma at points (3, B) with step h -> (3, B).  swap: the MUTANT that takes sigma at p- for sigma+ and the reverse, the
    denominator unchanged (tests only)."""
    p = np.ascontiguousarray(points, np.float32)
    B = p.shape[1]
    if B == 0:
        return np.zeros((3, 0), np.float32)
    st = stencil(p, h)
    sigma = np.asarray(density(st), np.float32)
    if swap:
        order = np.concatenate([np.arange((k ^ 1) * B, ((k ^ 1) + 1) * B) for k in range(6)])
        sigma = sigma[order]
    return _differences(st, sigma, B)


def ray_points(o, d, t):
    """x = fl(o + fl(d * t)) per coordinate for one ray: (3,), (3,), (n,) -> (3, n)."""
    prod = (np.asarray(d, np.float32)[:, None] * np.asarray(t, np.float32)[None, :]).astype(np.float32)
    return (np.asarray(o, np.float32)[:, None] + prod).astype(np.float32)


def ray_normals(density, o, d, t, w, h, swap=False, descending=False, live_ge=False, corrupt=None):
    """Per-ray normals: o (3,) or (R, 3) origins, d (R, 3) the directions the networks saw, t, w (R, n) the composited samples' positions
    and weights, h the step -> (R, 3) float32.
    A sample is live iff w > 0; G = sum over the live samples in ascending order of fl(w * g), n = (-G) / |G|, zero when |G| is 0 or not
    finite.  Mutants (tests only): swap (sigma at p- taken for sigma+ and the reverse), descending (the sum runs backwards), live_ge (live iff w >= 0); corrupt: a function
    (sigma of the stencil points (6 L,), weights of the L listed samples in list order) -> sigma, applied before the differences (to
    plant a non-finite sigma+ on chosen samples)."""
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    R = len(d)
    o = np.ascontiguousarray(o, np.float32)
    o = np.repeat(o[None, :], R, axis=0) if o.ndim == 1 else o
    t, w = np.asarray(t, np.float32), np.asarray(w, np.float32)
    live = (w >= 0) if live_ge else (w > 0)
    counts = live.sum(axis=1)
    L = int(counts.sum())
    out = np.zeros((R, 3), np.float32)
    if L == 0:
        return out
    pts = np.hstack([ray_points(o[r], d[r], t[r][live[r]]) for r in range(R)])
    st = stencil(pts, h)
    sigma = np.asarray(density(st), np.float32).copy()
    if corrupt is not None:
        sigma = np.asarray(corrupt(sigma, np.concatenate([w[r][live[r]] for r in range(R)])), np.float32)
    if swap:
        order = np.concatenate([np.arange((k ^ 1) * L, ((k ^ 1) + 1) * L) for k in range(6)])
        sigma = sigma[order]
    g = _differences(st, sigma, L)
    base = 0
    with np.errstate(all="ignore"):
        for r in range(R):
            wr = w[r][live[r]]
            order = range(len(wr) - 1, -1, -1) if descending else range(len(wr))
            G = [F(0.0), F(0.0), F(0.0)]
            for q in order:
                for a in range(3):
                    G[a] = F(G[a] + F(F(wr[q]) * F(g[a, base + q])))
            base += len(wr)
            length = np.sqrt(F(F(F(G[0] * G[0]) + F(G[1] * G[1])) + F(G[2] * G[2])))
            if np.isfinite(length) and length > 0:
                out[r] = [F(-G[a]) / length for a in range(3)]
    return out


def live_count(w):
    return int((np.asarray(w, np.float32) > 0).sum())


def angle_deg(a, b):
    """Angle between corresponding unit vectors (R, 3), degrees, in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.clip((a * b).sum(axis=1), -1.0, 1.0)
    return np.degrees(np.arccos(c))
