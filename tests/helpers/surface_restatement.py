"""Quantile depths and point clouds restated on the host (the contract: include/nerf_mi355x.h, "quantile depth and point clouds").

quantile_depths() walks a ray's compositing weights as k_ray_quantiles does -- cum = fl(cum + w_i) in ascending i, float32 -- and
returns per quantile q the position t_i of the first sample with cum_i >= q (0 where none is).  points() keeps the rays with
opacity >= min_opacity and a crossing, in ray order, and forms their records.  Both are NumPy float32 with an explicit loop over the
samples, vectorised over the rays, as ray_batch_restatement.sums_from_weights.  Nothing here looks at a rendered batch.

The keyword arguments of both functions are MUTANTS (tests/test_surface_restatement_cpu.py shows that each changes bits or indices); the
defaults are the contract."""
import numpy as np

F = np.float32


def cumulative(w):
    """cum (R, n): cum_i = fl(cum_{i-1} + w_i), cum_0 = +0, float32, ascending i."""
    w = np.ascontiguousarray(w, F)
    cum = np.empty_like(w)
    acc = np.zeros(w.shape[0], F)
    for i in range(w.shape[1]):
        acc = (acc + w[:, i]).astype(F)
        cum[:, i] = acc
    return cum


def quantile_depths(w, t, qs, return_index=False, strict=False, descending=False, next_sample=False):
    """w, t (R, n); qs: quantiles in (0, 1] -> depth_q (n_q, R) float32; return_index: also k (n_q, R) int64, -1 where no crossing.
    Mutants: strict (cum > q), descending (the walk runs from the last sample), next_sample (t_{k+1}, the last sample's own t at the end)."""
    w = np.ascontiguousarray(w, F)
    t = np.ascontiguousarray(t, F)
    R, n = w.shape
    qs = np.atleast_1d(np.asarray(qs, F))
    depth = np.zeros((len(qs), R), F)
    index = np.full((len(qs), R), -1, np.int64)
    pending = np.ones((len(qs), R), bool)
    acc = np.zeros(R, F)
    order = range(n - 1, -1, -1) if descending else range(n)
    with np.errstate(invalid="ignore"):
        for i in order:
            acc = (acc + w[:, i]).astype(F)
            for j, q in enumerate(qs):
                reached = pending[j] & ((acc > q) if strict else (acc >= q))     # a NaN sum compares false
                src = min(i + 1, n - 1) if next_sample else i
                depth[j, reached] = t[reached, src]
                index[j, reached] = i
                pending[j, reached] = False
    return (depth, index) if return_index else depth


def points(o, d, depth_q, C, A, normals, min_opacity, strict_keep=False):
    """o (3,) or (R, 3); d (R, 3) as the networks saw them; depth_q, A (R,); C (R, 3) the colour over black; normals (R, 3) or None.
    -> dict: n, ray (n,) uint32 ascending, xyz, rgb (n, 3), depth, opacity (n,), normals (n, 3) or absent.  Mutant: strict_keep
    (opacity > min_opacity)."""
    d = np.ascontiguousarray(d, F)
    R = len(d)
    o = np.ascontiguousarray(o, F)
    o = np.repeat(o[None, :], R, axis=0) if o.ndim == 1 else o
    depth_q = np.ascontiguousarray(depth_q, F)
    A = np.ascontiguousarray(A, F)
    C = np.ascontiguousarray(C, F)
    with np.errstate(invalid="ignore"):
        opaque = (A > F(min_opacity)) if strict_keep else (A >= F(min_opacity))
        keep = opaque & (depth_q != 0)
    ray = np.flatnonzero(keep).astype(np.uint32)
    dq = depth_q[keep]
    with np.errstate(all="ignore"):
        xyz = (o[keep] + (d[keep] * dq[:, None]).astype(F)).astype(F)
        rgb = (C[keep] / A[keep][:, None]).astype(F)
    out = dict(n=int(keep.sum()), ray=ray, xyz=xyz, rgb=rgb, depth=dq, opacity=A[keep])
    if normals is not None:
        out["normals"] = np.ascontiguousarray(normals, F)[keep]
    return out
