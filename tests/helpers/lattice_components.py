"""NumPy / plain-Python restatement of the lattice components (nerf_lattice_components and the filtered mesh entry points), written from the
definition in include/nerf_mi355x.h ("lattice components"), plus the synthetic fields the tests share.

Nothing here comes from the kernels: they label by union-find with atomics on the label array; this file floods each component from its
smallest index with an explicit stack over a padded lattice, and the mesh filter works on the finished unfiltered mesh of
helpers/marching_tets.py (it never classifies a cell)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marching_tets as MT  # noqa: E402

F = np.float32
NONE = 0xFFFFFFFF
KUHN_OFFSETS = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1) if (dx, dy, dz) != (0, 0, 0)]
NEIGHBOURS = KUHN_OFFSETS + [(-dx, -dy, -dz) for dx, dy, dz in KUHN_OFFSETS]     # 14: +d and -d for d in {0,1}^3 \ {0}
assert len(set(NEIGHBOURS)) == 14 and (1, 1, 1) in NEIGHBOURS and (1, -1, 0) not in NEIGHBOURS


def inside_mask(sigma, iso):
    with np.errstate(all="ignore"):
        return np.asarray(sigma, F) > F(iso)                  # a NaN is not inside, +inf is


def components(sigma, iso):
    """sigma (nz, ny, nx) -> (labels (nz, ny, nx) uint32, table): a component's label is the smallest linear index ix + nx (iy + ny iz) among
    its points, NONE where not inside; table = [(label, n_points, (ix_min, iy_min, iz_min, ix_max, iy_max, iz_max))] in rank order
    (n_points descending, ties by label ascending)."""
    ins = inside_mask(sigma, iso)
    nz, ny, nx = ins.shape
    px, py = nx + 2, ny + 2                                   # one layer of outside points all round: no bounds checks
    pad = np.zeros((nz + 2, py, px), bool)
    pad[1:-1, 1:-1, 1:-1] = ins
    todo = bytearray(pad.reshape(-1).tobytes())               # 1 = inside and not yet reached
    steps = [dx + px * (dy + py * dz) for dx, dy, dz in NEIGHBOURS]
    labels = np.full(nz * ny * nx, NONE, np.uint32)
    table = []
    iz, iy, ix = np.nonzero(ins)                              # ascending linear index: a new component is met at its smallest index first
    for sz, sy, sx in zip(iz.tolist(), iy.tolist(), ix.tolist()):
        start = (sx + 1) + px * ((sy + 1) + py * (sz + 1))
        if not todo[start]:
            continue
        todo[start] = 0
        stack, members = [start], []
        while stack:
            q = stack.pop()
            members.append(q)
            for s in steps:
                r = q + s
                if todo[r]:
                    todo[r] = 0
                    stack.append(r)
        m = np.asarray(members, np.int64)
        mx, my, mz = m % px - 1, (m // px) % py - 1, m // (px * py) - 1
        lin = mx + nx * (my + ny * mz)
        label = sx + nx * (sy + ny * sz)
        assert lin.min() == label
        labels[lin] = label
        table.append((int(label), int(m.size), (int(mx.min()), int(my.min()), int(mz.min()), int(mx.max()), int(my.max()), int(mz.max()))))
    table.sort(key=lambda e: (-e[1], e[0]))
    return labels.reshape(nz, ny, nx), table


def kept_labels(table, keep_largest, min_points):
    """The labels a filter keeps: n_points >= min_points and (keep_largest == 0 or rank < keep_largest)."""
    return [e[0] for rank, e in enumerate(table) if e[1] >= min_points and (keep_largest == 0 or rank < keep_largest)]


def filter_mesh(sigma, iso, vertices, normals, triangles, keep_largest, min_points, labelled=None):
    """The UNFILTERED mesh of marching_tets(sigma, ., ., iso) -> (vertices, normals, triangles, n_components, n_kept) of the filtered mesh: every
    vertex whose inside end lies in a discarded component goes, with every triangle that uses it; the rest keep their bits and their order,
    vertex ids are renumbered in their old order.  labelled: components(sigma, iso), if the caller has it already."""
    labels, table = labelled if labelled is not None else components(sigma, iso)
    kept = kept_labels(table, keep_largest, min_points)
    a, b = MT.vertex_edges(sigma, iso)
    assert len(a) == len(vertices)
    ins = inside_mask(sigma, iso)
    a_in = ins[a[:, 2], a[:, 1], a[:, 0]]
    assert (a_in != ins[b[:, 2], b[:, 1], b[:, 0]]).all()     # exactly one end of a vertex's edge is inside
    end = np.where(a_in[:, None], a, b)
    keep_v = np.isin(labels[end[:, 2], end[:, 1], end[:, 0]], np.asarray(kept, np.uint32))
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    tk = keep_v[t] if len(t) else np.zeros((0, 3), bool)
    assert (tk.all(axis=1) == tk.any(axis=1)).all()           # a triangle's vertices are all kept or all dropped
    new_id = np.cumsum(keep_v) - 1
    out_t = new_id[t[tk.all(axis=1)]].astype(np.uint32).reshape(-1, 3)
    return vertices[keep_v], None if normals is None else normals[keep_v], out_t, len(table), len(kept)


# ---- fields: sigma (nz, ny, nx) float32, inside where > 0 (iso 0); positions in index space -----------------------------------------------------
def _index_grid(dims):
    nx, ny, nz = dims
    iz, iy, ix = np.meshgrid(np.arange(nz, dtype=float), np.arange(ny, dtype=float), np.arange(nx, dtype=float), indexing="ij")
    return ix, iy, iz


FLOATER_BLOBS = [((15, 15, 14), 8.0), ((32, 6, 6), 3.2), ((32, 22, 20), 1.9), ((33, 14, 5), 2.6), ((5, 25, 24), 2.6)]   # the last two: equal sizes
FLOATER_POINTS = [(3, 3, 3),                                  # a single-point speck
                  (3, 3, 24), (4, 4, 25),                     # joined only by a body diagonal: one component
                  (36, 26, 3), (35, 27, 3)]                   # separated only by an anti-diagonal: two components


def floaters(dims):
    """A sphere, smaller blobs of different sizes, two blobs of equal size (integer centres, the same radius: the tie), a speck, a pair joined
    only by a body diagonal and a pair separated only by an anti-diagonal.  Laid out for lattices from 40 x 30 x 29; whatever does not fit
    wholly inside a smaller lattice is left out."""
    nx, ny, nz = dims
    ix, iy, iz = _index_grid(dims)
    s = np.full((nz, ny, nx), -1.0)
    for (cx, cy, cz), r in FLOATER_BLOBS:
        if cx + r + 1 < nx and cy + r + 1 < ny and cz + r + 1 < nz:
            s = np.maximum(s, r - np.sqrt((ix - cx) ** 2 + (iy - cy) ** 2 + (iz - cz) ** 2))
    for k, (x, y, z) in enumerate(FLOATER_POINTS):
        if x + 1 < nx and y + 1 < ny and z + 1 < nz:
            s[z, y, x] = 0.5 + 0.1 * k
    return s.astype(F)


def snake(dims):
    """One long one-point-wide component winding through the whole lattice: every second row of every second plane, consecutive rows joined at
    alternating ends, consecutive planes by one point.  Label chains are long and cross every workgroup; the root is index 0."""
    nx, ny, nz = dims
    s = np.full((nz, ny, nx), -1.0, F)
    for z in range(0, nz, 2):
        for y in range(0, ny, 2):
            s[z, y, :] = 1.0
            if y + 2 < ny:
                s[z, y + 1, nx - 1 if (y // 2) % 2 == 0 else 0] = 1.0
        if z + 2 < nz:
            s[z + 1, 0, 0] = 1.0
    return s


def hollow(dims):
    """A shell whose cavity is outside: one component with two surfaces."""
    nx, ny, nz = dims
    ix, iy, iz = _index_grid(dims)
    r2 = 0.42 * (min(dims) - 1)
    r1 = 0.55 * r2
    d = np.sqrt((ix - (nx - 1) / 2 - 0.13) ** 2 + (iy - (ny - 1) / 2 + 0.07) ** 2 + (iz - (nz - 1) / 2 - 0.21) ** 2)
    return np.minimum(r2 - d, d - r1).astype(F)


def noise(dims, p, seed):
    """Bernoulli(p) occupancy with random magnitudes: inside points in (0.1, 1.1), the others in (-1.1, -0.1)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    occ = rng.random((nz, ny, nx)) < p
    mag = 0.1 + rng.random((nz, ny, nx))
    return np.where(occ, mag, -mag).astype(F)
