"""include/pcm.h's contract of pcm_chamfer_nd_forward / pcm_chamfer_nd_backward
restated in numpy, and the input makers of the N-D Chamfer tests (a plain module
shared by tests/test_chamfer_nd_cpu.py and tests/test_chamfer_nd_gpu.py).

Distances and gradients of a correct kernel are EQUAL to these, bit for bit.
The fused step is formed in float64, where the product of two float32 values is
exact, and the float64 sum is rounded TO ODD before the cast to float32, so the
step rounds once: the plain float64 form rounds twice and differs from fmaf in
about 2^-29 of operations, and these tests make around 10^9 of them."""
import numpy as np


def fma_f32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, one rounding."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b  # exact: 48 significant bits
        s = p + c
        # TwoSum: s + err == p + c exactly
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (np.atleast_1d(s).view(np.int64) & 1).reshape(np.shape(s)) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)  # the odd neighbour on the residue's side
        return s.astype(np.float32)


def sqd_nd(x1, x2):
    """The pinned squared distances [n, m] float32 of float32 clouds x1 [n, D]
    (queries) and x2 [m, D] (candidates): c_t = x2[k][t] - x1[j][t], s = c_0 c_0,
    then s = fmaf(c_t, c_t, s)."""
    x1, x2 = np.asarray(x1, np.float32), np.asarray(x2, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = x2[None, :, 0] - x1[:, None, 0]
        s = (c * c).astype(np.float32)
        for t in range(1, x1.shape[1]):
            c = x2[None, :, t] - x1[:, None, t]
            s = fma_f32(c, c, s)
    return s


def nn_restated(x1, x2, rows=None):
    """dist [B, N] float32 and idx [B, N] int32 of direction 1 (queries x1
    [B, N, D], candidates x2 [B, M, D]); rows: only these query rows."""
    x1, x2 = np.asarray(x1, np.float32), np.asarray(x2, np.float32)
    if rows is not None:
        x1 = x1[:, rows]
    b, n, _ = x1.shape
    dist = np.empty((b, n), np.float32)
    idx = np.empty((b, n), np.int32)
    for bi in range(b):
        for r0 in range(0, n, 256):
            s = sqd_nd(x1[bi, r0:r0 + 256], x2[bi])
            key = np.where(np.isnan(s), np.float32(np.inf), s)
            k = np.argmin(key, axis=1)  # the first (lowest) index of the minimum
            idx[bi, r0:r0 + 256] = k
            dist[bi, r0:r0 + 256] = key[np.arange(key.shape[0]), k]
    return dist, idx


def forward_restated(x1, x2):
    """(dist1, dist2, idx1, idx2) of pcm_chamfer_nd_forward, both clouds non-empty."""
    d1, i1 = nn_restated(x1, x2)
    d2, i2 = nn_restated(x2, x1)
    return d1, d2, i1, i2


def _grad_one_cloud(self_, other, gd_self, idx_self, gd_other, idx_other, direct_first):
    f32 = np.float32
    ns, dim = self_.shape
    acc = np.zeros((ns, dim), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (gd_self * f32(2.0)).astype(f32)
        direct = (g[:, None] * (self_ - other[idx_self]).astype(f32)).astype(f32)
        if direct_first:
            acc = (acc + direct).astype(f32)
        for j in range(other.shape[0]):  # ascending: the pinned order
            i = idx_other[j]
            gj = f32(gd_other[j] * f32(2.0))
            acc[i] = (acc[i] + (-(gj * (other[j] - self_[i]).astype(f32)).astype(f32))).astype(f32)
        if not direct_first:
            acc = (acc + direct).astype(f32)
    return acc


def backward_restated(x1, x2, gd1, gd2, idx1, idx2):
    """(grad1, grad2) of pcm_chamfer_nd_backward on rows [B, N, D] / [B, M, D]."""
    x1, x2 = np.asarray(x1, np.float32), np.asarray(x2, np.float32)
    gd1, gd2 = np.asarray(gd1, np.float32), np.asarray(gd2, np.float32)
    g1, g2 = np.empty_like(x1), np.empty_like(x2)
    for bi in range(x1.shape[0]):
        g1[bi] = _grad_one_cloud(x1[bi], x2[bi], gd1[bi], idx1[bi], gd2[bi], idx2[bi], True)
        g2[bi] = _grad_one_cloud(x2[bi], x1[bi], gd2[bi], idx2[bi], gd1[bi], idx1[bi], False)
    return g1, g2


def make_cloud(rng, b, n, d, scale=1.0, shift=0.0):
    """[b, n, d] float32, uniform in [shift, shift + scale); every other point
    snapped to a lattice of scale / 4, so that exact ties occur."""
    x = rng.random((b, n, d), dtype=np.float32)
    x[:, ::2] = np.round(x[:, ::2] * 4) / 4
    return (x * np.float32(scale) + np.float32(shift)).astype(np.float32)


def make_clouds(seed, b, n, m, d, scale=1.0, shift=0.0):
    rng = np.random.default_rng(seed)
    return make_cloud(rng, b, n, d, scale, shift), make_cloud(rng, b, m, d, scale, shift)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)
