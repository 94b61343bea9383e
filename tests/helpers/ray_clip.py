"""NumPy restatement of ray clipping (include/nerf_mi355x.h, "ray clipping"): nerf_occupancy_dilate and nerf_clip_rays, every step in
np.float32 in the order the header gives (one rounding per operation; numpy never contracts), vectorised over the rays.  Beside it an
independent float64 brute force (every occupied cell's box against every ray) and the ray / grid cases the CPU and GPU tests share."""
import numpy as np

F = np.float32


def _max(a, b):  # the header's max: a NaN in a is dropped, one in b is kept
    return np.where(a > b, a, b)


def _min(a, b):
    return np.where(a < b, a, b)


# ---- occupancy words ---------------------------------------------------------------------------------------------------------------------
def pack(occ):
    """bool (nz, ny, nx) -> ceil(N / 32) uint32 words: bit b of word w is linear cell 32 w + b, x fastest; the bits behind N - 1 are 0."""
    flat = np.ascontiguousarray(occ, dtype=bool).reshape(-1)
    pad = (-flat.size) % 32
    return np.packbits(np.concatenate([flat, np.zeros(pad, bool)]), bitorder="little").view("<u4").astype(np.uint32)


def unpack(bits, dims):
    nx, ny, nz = (int(v) for v in dims)
    words = np.ascontiguousarray(bits, dtype="<u4").reshape(-1)
    assert words.size == (nx * ny * nz + 31) // 32
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:nx * ny * nz].astype(bool).reshape(nz, ny, nx)


def dilate(bits, dims, radius):
    """A cell is set iff any input cell within Chebyshev distance radius, inside the grid, is set -> (words, count, bounds)."""
    occ = unpack(bits, dims)
    nz, ny, nx = occ.shape
    out = np.zeros_like(occ)
    r = int(radius)
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                # out[z, y, x] |= occ[z + dz, y + dy, x + dx] where that cell exists
                z0, z1 = max(0, -dz), min(nz, nz - dz)
                y0, y1 = max(0, -dy), min(ny, ny - dy)
                x0, x1 = max(0, -dx), min(nx, nx - dx)
                if z0 < z1 and y0 < y1 and x0 < x1:
                    out[z0:z1, y0:y1, x0:x1] |= occ[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return pack(out), int(out.sum()), occupancy_bounds(out)


def occupancy_bounds(occ):
    """nerf_density_grid's bounds: inclusive (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max); no set cell: mins = dims, maxs = -1."""
    nz, ny, nx = occ.shape
    if not occ.any():
        return (nx, ny, nz, -1, -1, -1)
    z, y, x = np.nonzero(occ)
    return (int(x.min()), int(y.min()), int(z.min()), int(x.max()), int(y.max()), int(z.max()))


# ---- the clip ------------------------------------------------------------------------------------------------------------------------------
def directions(dirs, normalize=True):
    d = np.ascontiguousarray(dirs, F)
    if not normalize:
        return d.copy()
    with np.errstate(all="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return (d / length[:, None]).astype(F)


def _plane(g_lo, st, k):
    return g_lo + st * k.astype(F)


def _crossing(g_lo, st, i, s, o, inv):
    with np.errstate(all="ignore"):
        t = (_plane(g_lo, st, i + (s > 0)) - o) * inv
    return np.where(s == 0, F(np.inf), t).astype(F)


def _entry(q, n):
    f = np.floor(q)
    i = np.where(f >= F(n - 1), n - 1, np.where(f > 0, f, 0))           # comparisons: +-inf and NaN never reach the conversion
    i = np.where(np.isnan(q), 0, i)
    return np.nan_to_num(i, nan=0.0, posinf=n - 1, neginf=0).astype(np.int64)


def clip_rays(bits, lo, step, dims, origins, dirs, near, far, bounds=None, normalize=True, return_rounds=False):
    """-> (bounds_out (n, 2) float32, hit (n,) bool[, rounds (n,)])"""
    dims = [int(v) for v in dims]
    lo, step = np.asarray(lo, F), np.asarray(step, F)
    occ = unpack(bits, dims).reshape(-1)
    d = directions(dirs, normalize)
    n = d.shape[0]
    o = np.ascontiguousarray(origins, F)
    o = np.broadcast_to(o.reshape(1, 3), (n, 3)) if o.ndim == 1 or o.shape[0] == 1 and n != 1 else o
    if bounds is None:
        near_r, far_r = np.full(n, near, F), np.full(n, far, F)
    else:
        b = np.ascontiguousarray(bounds, F)
        near_r, far_r = b[:, 0].copy(), b[:, 1].copy()
    with np.errstate(all="ignore"):
        g_lo = [lo[a] - F(0.5) * step[a] for a in range(3)]
        g_hi = [lo[a] + step[a] * (F(dims[a]) - F(0.5)) for a in range(3)]
        t_in, t_out = near_r.copy(), far_r.copy()
        miss = np.zeros(n, bool)
        inv = []
        for a in range(3):
            oa, da = o[:, a], d[:, a]
            zero = da == 0
            miss |= zero & ~((g_lo[a] <= oa) & (oa < g_hi[a]))
            inv_a = (F(1.0) / np.where(zero, F(1.0), da)).astype(F)
            ta, tb = (g_lo[a] - oa) * inv_a, (g_hi[a] - oa) * inv_a
            t_in = np.where(zero, t_in, _max(t_in, _min(ta, tb)))
            t_out = np.where(zero, t_out, _min(t_out, _max(ta, tb)))
            inv.append(np.where(zero, F(0.0), inv_a).astype(F))
        miss |= ~(t_in < t_out)
        i = [_entry(((o[:, a] + d[:, a] * t_in) - g_lo[a]) / step[a], dims[a]) for a in range(3)]
        s = [np.where(d[:, a] > 0, 1, np.where(d[:, a] < 0, -1, 0)).astype(np.int64) for a in range(3)]
        tn = [_crossing(g_lo[a], step[a], i[a], s[a], o[:, a], inv[a]) for a in range(3)]
        t_cur = t_in.copy()
        t_first, t_last = np.zeros(n, F), np.zeros(n, F)
        hit = np.zeros(n, bool)
        alive = ~miss
        rounds = np.zeros(n, np.int64)
        for _ in range(dims[0] + dims[1] + dims[2] + 3):
            if not alive.any():
                break
            rounds += alive
            ax = np.zeros(n, np.int64)
            m = tn[0].copy()
            for a in (1, 2):
                better = tn[a] < m
                ax = np.where(better, a, ax)
                m = np.where(better, tn[a], m)
            t_exit = _min(m, t_out)
            cell = i[0] + dims[0] * (i[1] + dims[1] * i[2])
            assert np.all((cell[alive] >= 0) & (cell[alive] < occ.size))       # no cell outside the grid is ever looked at
            inside = alive & occ[np.where(alive, cell, 0)] & (t_exit > t_cur)
            t_first = np.where(inside & ~hit, t_cur, t_first)
            t_last = np.where(inside, t_exit, t_last)
            hit |= inside
            alive &= ~(t_out <= m)
            for a in range(3):
                move = alive & (ax == a)
                i[a] = np.where(move, i[a] + s[a], i[a])
                alive &= ~(move & ((i[a] < 0) | (i[a] >= dims[a])))
            t_cur = np.where(alive, _max(t_cur, m), t_cur)
            for a in range(3):
                move = alive & (ax == a)
                tn[a] = np.where(move, _crossing(g_lo[a], step[a], np.clip(i[a], 0, dims[a] - 1), s[a], o[:, a], inv[a]), tn[a])
    out = np.stack([np.where(hit, t_first, near_r), np.where(hit, t_last, far_r)], axis=1).astype(F)
    return (out, hit, rounds) if return_rounds else (out, hit)


# ---- the independent reference: float64, every occupied cell against every ray ---------------------------------------------------------------
def brute_force(bits, lo, step, dims, origins, d_unit, near_r, far_r):
    """d_unit: the directions the walk sees (float32, already normalised), taken as exact.  Per ray the slab intersection of [near, far] with
    the box of every occupied cell (exact boxes lo + step (i -+ 1/2) in float64; an axis with d = 0 uses the half-open rule) ->
    dict(t_first, t_last: min / max over the cells with a positive intersection; longest: the longest signed intersection over the
    occupied cells (-inf without one), t_at_longest: the larger |t| of that intersection)."""
    occ = unpack(bits, dims)
    z, y, x = np.nonzero(occ)
    idx = np.stack([x, y, z], axis=1).astype(np.float64)                                       # (c, 3)
    lo64, st64 = np.asarray(lo, F).astype(np.float64), np.asarray(step, F).astype(np.float64)
    b_lo, b_hi = lo64 + st64 * (idx - 0.5), lo64 + st64 * (idx + 0.5)
    o = np.ascontiguousarray(origins, F).astype(np.float64)
    d = np.ascontiguousarray(d_unit, F).astype(np.float64)
    n = d.shape[0]
    o = np.broadcast_to(o.reshape(-1, 3), (n, 3))
    t0 = np.broadcast_to(np.asarray(near_r, np.float64)[:, None], (n, idx.shape[0])).copy()
    t1 = np.broadcast_to(np.asarray(far_r, np.float64)[:, None], (n, idx.shape[0])).copy()
    with np.errstate(all="ignore"):
        for a in range(3):
            da, oa = d[:, a:a + 1], o[:, a:a + 1]
            zero = da == 0
            ta, tb = (b_lo[None, :, a] - oa) / np.where(zero, 1.0, da), (b_hi[None, :, a] - oa) / np.where(zero, 1.0, da)
            inside = (b_lo[None, :, a] <= oa) & (oa < b_hi[None, :, a])
            t0 = np.where(zero, np.where(inside, t0, np.inf), np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(zero, np.where(inside, t1, -np.inf), np.minimum(t1, np.maximum(ta, tb)))
    length = t1 - t0
    if idx.shape[0] == 0:
        return dict(hit=np.zeros(n, bool), t_first=np.zeros(n), t_last=np.zeros(n), longest=np.full(n, -np.inf), t_at_longest=np.zeros(n))
    pos = length > 0
    k = np.argmax(np.where(np.isnan(length), -np.inf, length), axis=1)
    rows = np.arange(n)
    return dict(hit=pos.any(axis=1), t_first=np.where(pos, t0, np.inf).min(axis=1), t_last=np.where(pos, t1, -np.inf).max(axis=1),
                longest=length[rows, k], t_at_longest=np.maximum(np.abs(t0[rows, k]), np.abs(t1[rows, k])))


def tolerance(lo, step, dims, origins, d_unit, t):
    """tol_r = 4 * 2^-24 * ((|P|max + |o_r|inf) / min_{d_a != 0} |d_a| + |t|): a plane and the origin are each within half an ulp of their
    size, their difference and the product with 1 / d add three more roundings of that size, all divided by |d_a|; t itself carries one."""
    lo64, st64 = np.asarray(lo, np.float64), np.asarray(step, np.float64)
    p_max = np.max(np.maximum(np.abs(lo64 - 0.5 * st64), np.abs(lo64 + st64 * (np.asarray(dims) - 0.5))))
    d = np.abs(np.asarray(d_unit, np.float64))
    n = d.shape[0]
    o = np.broadcast_to(np.abs(np.asarray(origins, np.float64)).reshape(-1, 3), (n, 3))
    d_min = np.where(d == 0, np.inf, d).min(axis=1)
    return 4.0 * 2.0 ** -24 * ((p_max + o.max(axis=1)) / d_min + np.abs(t))


# ---- shared cases ----------------------------------------------------------------------------------------------------------------------------
GRID_DIMS, GRID_STEP, GRID_LO = (13, 9, 11), (0.21, 0.19, 0.17), (-1.3, -0.8, -0.9)


def random_grid(dims, share, seed):
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    return pack(rng.random((nz, ny, nx)) < share)


def shell_grid(n=40, thick=2, inner=8):
    """n^3 with a `thick`-cell shell occupied: the cells whose Chebyshev distance from the cube [inner, n - inner) is 1 .. thick"""
    c = np.arange(n)
    dist = np.maximum(np.maximum(inner - c, c - (n - inner - 1)), 0)
    cheb = np.maximum(np.maximum(dist[:, None, None], dist[None, :, None]), dist[None, None, :])
    return pack((cheb >= 1) & (cheb <= thick))


def make_rays(lo, step, dims, n=3000, n_zero=250, seed=11):
    """n rays around the grid lo, step, dims -> dict(origins (n, 3), dirs (n, 3; not unit), bounds (n, 2)):
    origins inside and outside the grid, directions towards random points of the grid, n_zero rays with one or two direction
    components exactly 0, a quarter of the rays with their own short {near, far}."""
    rng = np.random.default_rng(seed)
    lo, step, dims = np.asarray(lo, np.float64), np.asarray(step, np.float64), np.asarray(dims, np.float64)
    g_lo, g_hi = lo - 0.5 * step, lo + step * (dims - 0.5)
    centre, half = 0.5 * (g_lo + g_hi), 0.5 * (g_hi - g_lo)
    inside = rng.random(n) < 0.4
    o_in = rng.uniform(g_lo, g_hi, (n, 3))
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o_out = centre + v * np.linalg.norm(half) * rng.uniform(1.2, 3.0, (n, 1))
    origins = np.where(inside[:, None], o_in, o_out).astype(F)
    target = rng.uniform(g_lo - 0.1 * half, g_hi + 0.1 * half, (n, 3))
    dirs = (target - origins).astype(F)
    zero = rng.choice(n, n_zero, replace=False)
    for k, r in enumerate(zero):                                          # one or two components exactly 0
        axes = rng.permutation(3)[:1 + k % 2]
        dirs[r, axes] = 0.0
        if k % 3:                                                         # most of them from inside the slab of the zeroed axes
            origins[r, axes] = rng.uniform(g_lo[axes], g_hi[axes]).astype(F)
    dist = np.linalg.norm(centre - origins, axis=1)
    bounds = np.stack([np.zeros(n), dist + np.linalg.norm(half) * 1.5], axis=1)
    short = rng.random(n) < 0.25
    near_s = rng.uniform(0.0, 1.0, n) * (dist + np.linalg.norm(half))
    bounds[short, 0] = near_s[short]
    bounds[short, 1] = near_s[short] + rng.uniform(0.05, 0.6, n)[short]
    return dict(origins=origins, dirs=dirs, bounds=bounds.astype(F))
