"""NumPy restatement of the isosurface extraction (nerf_isosurface_grid / nerf_extract_mesh), written from the conventions in
include/nerf_mi355x.h ("isosurface meshes"), plus the synthetic fields and mesh invariants the tests share.

Nothing here comes from the kernel: the kernel decides a triangle's winding from permutation parities, this file from geometry -- it places
the vertices of each configuration at the edge midpoints in index space, takes the normal of the polygon and compares it with the direction
from the inside corners to the outside corners.  All vertex arithmetic is float32, one NumPy operation per rounding."""
import itertools

import numpy as np

F = np.float32
AXIS_ORDERS = list(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx: (a, b, c)
assert AXIS_ORDERS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
EDGE_OFFSETS = [(e & 1, (e >> 1) & 1, e >> 2) for e in range(8)]   # e = dx + 2 dy + 4 dz -> (dx, dy, dz)


def lattice_axes(lo, step, dims):
    """x_k(i) = lo_k + step_k * (float)i: product, then sum, each rounded once."""
    return [(F(lo[k]) + F(step[k]) * np.arange(dims[k], dtype=F)).astype(F) for k in range(3)]


def _tet_corners(order):
    a, b, _ = order
    c0 = np.zeros(3, int); c1 = c0.copy(); c1[a] = 1; c2 = c1.copy(); c2[b] = 1
    return [c0, c1, c2, np.ones(3, int)]


def _polygon(corners, inside):
    """The polygon of one tetrahedron configuration as a list of corner-index pairs (each an edge with one end inside), in cyclic order,
    counter-clockwise seen from the outside in index space."""
    ins = [i for i in range(4) if inside[i]]
    outs = [i for i in range(4) if not inside[i]]
    if len(ins) == 1:
        cyc = [(ins[0], o) for o in outs]
    elif len(ins) == 3:
        cyc = [(i, outs[0]) for i in ins]
    else:                                                      # neighbours in the cycle share a face of the tetrahedron
        cyc = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
    mid = [(corners[i] + corners[j]) / 2.0 for i, j in cyc]
    normal = np.cross(mid[1] - mid[0], mid[-1] - mid[0])
    outward = np.mean([corners[o] for o in outs], axis=0) - np.mean([corners[i] for i in ins], axis=0)
    d = float(np.dot(normal, outward))
    assert abs(d) > 1e-9
    return cyc if d > 0 else [cyc[0]] + cyc[:0:-1]


def _gradient(sigma, axes):
    """g[..., k] = (sigma(P + e_k) - sigma(P - e_k)) / (x_k(P + e_k) - x_k(P - e_k)), indices clamped to the lattice."""
    nz, ny, nx = sigma.shape
    g = np.empty(sigma.shape + (3,), F)
    for k, (n, axis) in enumerate(((nx, 2), (ny, 1), (nz, 0))):
        i = np.arange(n)
        ip, im = np.minimum(i + 1, n - 1), np.maximum(i - 1, 0)
        ds = (np.take(sigma, ip, axis=axis) - np.take(sigma, im, axis=axis)).astype(F)
        dx = (axes[k][ip] - axes[k][im]).astype(F)
        shape = [1, 1, 1]; shape[axis] = n
        g[..., k] = ds / dx.reshape(shape)
    return g


def marching_tets(sigma, lo, step, iso):
    """sigma (nz, ny, nx) float32 -> (vertices (V, 3) f32, normals (V, 3) f32, triangles (T, 3) uint32)."""
    sigma = np.ascontiguousarray(sigma, dtype=F)
    nz, ny, nx = sigma.shape
    assert min(nx, ny, nz) >= 2
    iso = F(iso)
    axes = lattice_axes(lo, step, (nx, ny, nz))
    with np.errstate(all="ignore"):
        inside = sigma > iso                                   # a NaN is not inside
        finite = np.isfinite(sigma)
        # ---- vertices: has[A, e], ids ascending with A, within A with e
        has = np.zeros((nz, ny, nx, 8), bool)
        for e in range(1, 8):
            dx, dy, dz = EDGE_OFFSETS[e]
            A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
            B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
            has[A + (e,)] = finite[A] & finite[B] & (inside[A] != inside[B])
        vid = np.cumsum(has.reshape(-1)).reshape(has.shape) - 1
        vid[~has] = -1
        iz, iy, ix, e = np.nonzero(has)                        # C order: ascending A, then e
        dxs, dys, dzs = e & 1, (e >> 1) & 1, e >> 2
        sa, sb = sigma[iz, iy, ix], sigma[iz + dzs, iy + dys, ix + dxs]
        t = ((iso - sa).astype(F) / (sb - sa).astype(F)).astype(F)
        pa = np.stack([axes[0][ix], axes[1][iy], axes[2][iz]], axis=1)
        pb = np.stack([axes[0][ix + dxs], axes[1][iy + dys], axes[2][iz + dzs]], axis=1)
        vertices = (pa + (t[:, None] * (pb - pa).astype(F)).astype(F)).astype(F)
        g = _gradient(sigma, axes)
        ga, gb = g[iz, iy, ix], g[iz + dzs, iy + dys, ix + dxs]
        gv = (ga + (t[:, None] * (gb - ga).astype(F)).astype(F)).astype(F)
        sq = (gv * gv).astype(F)
        length = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)).astype(F)
        ok = np.isfinite(length) & (length != 0)
        normals = np.where(ok[:, None], ((-gv) / length[:, None]).astype(F), F(0)).astype(F)
    # ---- triangles: cells in linear order, six tetrahedra each, one triangle or one quad (two triangles) per tetrahedron
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cz, cy, cx = cz.ravel(), cy.ravel(), cx.ravel()            # ascending linear cell index ix + (nx - 1)(iy + (ny - 1) iz)
    valid = np.ones(cz.size, bool)
    for dx, dy, dz in EDGE_OFFSETS:
        valid &= finite[cz + dz, cy + dy, cx + dx]
    tris, keys = [], []
    for ti, order in enumerate(AXIS_ORDERS):
        corners = _tet_corners(order)
        ins = np.stack([inside[cz + c[2], cy + c[1], cx + c[0]] for c in corners], axis=1)      # (cells, 4)
        pattern = ins[:, 0] * 1 + ins[:, 1] * 2 + ins[:, 2] * 4 + ins[:, 3] * 8
        for pat in range(1, 15):
            sel = np.flatnonzero(valid & (pattern == pat))
            if sel.size == 0:
                continue
            cyc = _polygon(corners, [(pat >> i) & 1 for i in range(4)])
            ids = []
            for i, j in cyc:                                   # the edge is owned by the corner that comes first in the chain c0 < c1 < c2 < c3
                lo_c, hi_c = (i, j) if i < j else (j, i)
                d = corners[hi_c] - corners[lo_c]
                own = corners[lo_c]
                ids.append(vid[cz[sel] + own[2], cy[sel] + own[1], cx[sel] + own[0], d[0] + 2 * d[1] + 4 * d[2]])
            ids = np.stack(ids, axis=1)
            assert (ids >= 0).all()
            r = np.argmin(ids, axis=1)                         # canonical form: start at the smallest id, keep the cyclic order
            n = ids.shape[1]
            rolled = np.stack([ids[np.arange(sel.size), (r + k) % n] for k in range(n)], axis=1)
            for sub in range(n - 2):                           # (m, q1, q2) [, (m, q2, q3)]
                tris.append(rolled[:, [0, sub + 1, sub + 2]])
                keys.append(np.stack([sel, np.full(sel.size, ti), np.full(sel.size, sub)], axis=1))
    if not tris:
        return vertices, normals, np.zeros((0, 3), np.uint32)
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return vertices, normals, tris[order].astype(np.uint32)


def vertex_edges(sigma, iso):
    """Per vertex (in id order) the lattice indices of its edge's two ends: (A (V, 3), B (V, 3)) as (ix, iy, iz)."""
    sigma = np.asarray(sigma, F)
    nz, ny, nx = sigma.shape
    with np.errstate(all="ignore"):
        inside, finite = sigma > F(iso), np.isfinite(sigma)
    has = np.zeros((nz, ny, nx, 8), bool)
    for e in range(1, 8):
        dx, dy, dz = EDGE_OFFSETS[e]
        A = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        B = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        has[A + (e,)] = finite[A] & finite[B] & (inside[A] != inside[B])
    iz, iy, ix, e = np.nonzero(has)
    a = np.stack([ix, iy, iz], axis=1)
    return a, a + np.stack([e & 1, (e >> 1) & 1, e >> 2], axis=1)


# ---- synthetic fields: sigma (nz, ny, nx) float32 on the lattice, "inside" where the value exceeds iso -----------------------------------
def lattice_grid(lo, step, dims):
    ax = lattice_axes(lo, step, dims)
    z, y, x = np.meshgrid(ax[2].astype(np.float64), ax[1].astype(np.float64), ax[0].astype(np.float64), indexing="ij")
    return x, y, z


def unit_lattice(dims, margin=0.0):
    """lo, step of a lattice that spans [-1 - margin, 1 + margin]^3 with dims points per axis."""
    lo = np.full(3, -1.0 - margin)
    step = (2.0 + 2 * margin) / (np.asarray(dims, float) - 1)
    return F(lo), F(step)


def sphere_field(lo, step, dims, centre=(0.03, -0.02, 0.05), radius=0.71):
    x, y, z = lattice_grid(lo, step, dims)
    c = np.asarray(centre, float)
    return (radius - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)).astype(F)      # iso 0; gradient = -(p - c) / |p - c|


def two_spheres_field(lo, step, dims):
    x, y, z = lattice_grid(lo, step, dims)
    d1 = 0.36 - np.sqrt((x + 0.5) ** 2 + (y + 0.05) ** 2 + (z - 0.02) ** 2)
    d2 = 0.33 - np.sqrt((x - 0.52) ** 2 + (y - 0.04) ** 2 + (z + 0.03) ** 2)
    return np.maximum(d1, d2).astype(F)


def torus_field(lo, step, dims, major=0.6, minor=0.26):
    x, y, z = lattice_grid(lo, step, dims)
    q = np.sqrt((x - 0.01) ** 2 + (y + 0.02) ** 2) - major
    return (minor - np.sqrt(q ** 2 + (z - 0.015) ** 2)).astype(F)


def plane_field(lo, step, dims, normal=(0.3, -0.5, 0.81), offset=0.07):
    x, y, z = lattice_grid(lo, step, dims)
    n = np.asarray(normal, float) / np.linalg.norm(normal)
    return (offset - (n[0] * x + n[1] * y + n[2] * z)).astype(F)


def integer_field(dims, through=(2, 1, 1)):
    """r2 - |index - centre|^2 in doubled coordinates (2 i - (n - 1): integers whatever the parity of n), with r2 the squared distance of
    the lattice point `through` index steps away from the middle index (clamped to the lattice): an integer-valued field whose level set 0
    passes exactly through lattice points, so that sigma == iso occurs at corners."""
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d2 = (2 * ix - (nx - 1)) ** 2 + (2 * iy - (ny - 1)) ** 2 + (2 * iz - (nz - 1)) ** 2
    at = [min(n // 2 + o, n - 1) for n, o in zip(dims, through)]
    return (d2[at[2], at[1], at[0]] - d2).astype(F)


# ---- invariants ---------------------------------------------------------------------------------------------------------------------------
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_manifold(triangles):
    """Every undirected index edge lies in exactly two triangles and is traversed once in each direction."""
    e = directed_edges(triangles)
    if e.size == 0:
        return False
    if (e[:, 0] == e[:, 1]).any():
        return False
    key = e[:, 0] * (e.max() + 1) + e[:, 1]
    rev = e[:, 1] * (e.max() + 1) + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).all() and np.array_equal(uniq, np.unique(rev)))


def euler_characteristic(n_vertices, triangles):
    e = np.sort(directed_edges(triangles), axis=1)
    n_edges = np.unique(e, axis=0).shape[0]
    used = np.unique(np.asarray(triangles)).size
    assert used == n_vertices, (used, n_vertices)              # no vertex is left unused
    return n_vertices - n_edges + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.sum(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2]))) / 6.0)


def triangle_normals_and_centroids(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), v.mean(axis=1)
