"""include/pcm.h's contracts of pcm_knn and pcm_repulsion_loss restated in numpy
(a plain module shared by tests/test_knn_cpu.py and tests/test_knn_gpu.py).

The distance is the library's pinned float32 expression, formed exactly (each
fused step in float64, where the product is exact, and rounded once), and the
list is a (d, j) lexsort: indices and distance bits of a correct kernel are
EQUAL to these, not close."""
import numpy as np


def sqd_pinned(dx, dy, dz):
    """fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on float32 arrays."""
    dx, dy, dz = (np.asarray(v, np.float32) for v in (dx, dy, dz))
    t = (dx * dx).astype(np.float32)
    t = (dy.astype(np.float64) * dy + t).astype(np.float32)
    return (dz.astype(np.float64) * dz + t).astype(np.float32)


def knn_restated(query, ref, k, rows=None):
    """dist [B, N, k] float32 and idx [B, N, k] int32 of pcm_knn for float32
    clouds query [B, N, 3] and ref [B, M, 3]; rows: only these query rows."""
    query, ref = np.asarray(query, np.float32), np.asarray(ref, np.float32)
    if rows is not None:
        query = query[:, rows]
    b, n, _ = query.shape
    m = ref.shape[1]
    dist = np.full((b, n, k), np.inf, np.float32)
    idx = np.full((b, n, k), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(b):
            diff = ref[bi][None, :, :] - query[bi][:, None, :]  # float32: ref_j - query_i
            d = sqd_pinned(diff[..., 0], diff[..., 1], diff[..., 2])
            d = np.where(np.isfinite(d), d, np.float32(np.inf))  # NaN and +inf are never listed
            order = np.argsort(d, axis=1, kind="stable")[:, :k]  # equal d: the lower j first
            got = np.take_along_axis(d, order, axis=1)
            keep = min(k, m)
            dist[bi, :, :keep] = got
            idx[bi, :, :keep] = np.where(np.isfinite(got), order, -1)
    return dist, idx


def repulsion_terms(dist, h):
    """The float32 terms h - d of slots 1..4 and which of them are active."""
    terms = (np.float32(h) - np.asarray(dist, np.float32)[:, :, 1:5]).astype(np.float32)
    return terms, terms > 0


def repulsion_restated(xyz, h):
    """(loss, active share, dist, idx): the loss as the float64 sum of the
    float32 terms over 4 b n, from the restated k = 5 self search."""
    xyz = np.asarray(xyz, np.float32)
    b, n, _ = xyz.shape
    dist, idx = knn_restated(xyz, xyz, 5)
    terms, active = repulsion_terms(dist, h)
    loss = terms[active].astype(np.float64).sum() / (4.0 * b * n)
    return loss, float(active.mean()), dist, idx


def repulsion_gradient_f64(xyz, dist, idx, h):
    """The contract's gradient in float64 over the given lists, with what its
    float32 error bound needs: (grad [B, N, 3], T [B, N] terms per point,
    S [B, N, 3] sum of the terms' magnitudes per component)."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    b, n, _ = p.shape
    c = 2.0 / (4.0 * b * n)
    _, active = repulsion_terms(dist, h)
    grad = np.zeros((b, n, 3))
    mag = np.zeros((b, n, 3))
    count = np.zeros((b, n))
    for bi in range(b):
        i, t = np.nonzero(active[bi])
        j = np.asarray(idx)[bi, i, t + 1].astype(np.int64)
        diff = c * (p[bi, i] - p[bi, j])
        np.add.at(grad[bi], i, -diff)
        np.add.at(grad[bi], j, diff)
        np.add.at(mag[bi], i, np.abs(diff))
        np.add.at(mag[bi], j, np.abs(diff))
        np.add.at(count[bi], i, 1)
        np.add.at(count[bi], j, 1)
    return grad, count, mag


def gradient_bound(count, mag):
    """(T + 4) 2^-23 S per component: T float32 differences (2^-24 each), their
    T - 1 float32 additions, the rounding of the weight 2 / (4 b n) and the
    final product, with a factor two to spare -- derived, not measured."""
    return (count[..., None] + 4.0) * 2.0 ** -23 * mag
