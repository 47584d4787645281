"""include/pcm.h's contracts of pcm_ball_query and pcm_uniform_loss restated in
numpy (a plain module shared by tests/test_uniform_cpu.py and
tests/test_uniform_gpu.py), with the pcm_fps rule they build on.

Distances are the library's pinned float32 expression (knn_restated.sqd_pinned),
so the index lists of a correct kernel are EQUAL to these; the loss is float64
arithmetic over the float32 u values and the gradient float64 over the float32
roots, which a correct kernel matches within the derived bounds below."""
import math

import numpy as np

from knn_restated import knn_restated, sqd_pinned

F32 = np.float32


def make_cloud(kind, b, n, seed):
    """The test clouds: 'cube' is rand in [0, 1)^3, 'shell' normalised Gaussian
    directions scaled to radius 0.5."""
    rng = np.random.default_rng(seed)
    if kind == "cube":
        return rng.random((b, n, 3), dtype=F32)
    g = rng.standard_normal((b, n, 3))
    return (0.5 * g / np.linalg.norm(g, axis=2, keepdims=True)).astype(F32)


def uniform_params(n, percentage, radius=1.0):
    """(npoint, nsample, ball_radius, weight, expect_len) as Loss.get_uniform_loss forms them."""
    npoint = int(n * 0.05)
    nsample = [int(n * p) for p in percentage]
    ball_radius = [math.sqrt(p * radius) for p in percentage]
    weight = [math.pow(p * 100, 2) / len(percentage) for p in percentage]
    return npoint, nsample, ball_radius, weight, math.sqrt(math.pi * radius ** 2 / n)


def fps_restated(xyz, npoint, start=0):
    """idx [B, npoint] int64 of pcm_fps: running minima from 1e10f, a NaN
    distance changes nothing, the lowest index attaining the maximum is next."""
    xyz = np.asarray(xyz, F32)
    b, n, _ = xyz.shape
    idx = np.zeros((b, npoint), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(b):
            p = xyz[bi]
            run = np.full(n, 1e10, F32)
            far = start
            for i in range(npoint):
                idx[bi, i] = far
                diff = p - p[far]
                d = sqd_pinned(diff[:, 0], diff[:, 1], diff[:, 2])
                run = np.where(d < run, d, run)
                far = int(np.argmax(run))  # the first index attaining the maximum
    return idx


def ball_query_restated(xyz, new_xyz, radius, nsample):
    """(idx [B, S, nsample] int32, cnt [B, S] int32, hits [B, S]): the first
    nsample hits (d < fl(radius^2)) in ascending index, the first hit repeated
    behind them, zeros without a hit; cnt = min(hits, nsample); hits uncapped."""
    xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
    b, n, _ = xyz.shape
    s = new_xyz.shape[1]
    r2 = F32(F32(radius) * F32(radius))
    idx = np.zeros((b, s, nsample), np.int32)
    cnt = np.zeros((b, s), np.int32)
    hits = np.zeros((b, s), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(b):
            diff = xyz[bi][None, :, :] - new_xyz[bi][:, None, :]  # float32: point_k - centre_c
            d = sqd_pinned(diff[..., 0], diff[..., 1], diff[..., 2])
            inside = d < r2  # NaN is never a hit; exactly r2 is outside
            for c in range(s):
                h = np.nonzero(inside[c])[0]
                hits[bi, c] = len(h)
                k = min(len(h), nsample)
                cnt[bi, c] = k
                if k:
                    idx[bi, c, :k] = h[:k]
                    idx[bi, c, k:] = h[0]
    return idx, cnt, hits


def gather_points(xyz, idx):
    """xyz[b, idx[b, ...], :] for idx [B, ...]."""
    xyz = np.asarray(xyz)
    return np.stack([xyz[bi][np.asarray(idx)[bi]] for bi in range(xyz.shape[0])])


def uniform_groups(xyz, npoint, nsample, ball_radius):
    """(seeds [B, npoint], groups: per scale idx [B, npoint, nsample[q]] int32,
    hits: per scale [B, npoint] uncapped counts)."""
    seeds = fps_restated(xyz, npoint, 0)
    centres = gather_points(xyz, seeds)
    groups, hits = [], []
    for ns, r in zip(nsample, ball_radius):
        g, _, h = ball_query_restated(xyz, centres, r, ns)
        groups.append(g)
        hits.append(h)
    return seeds, groups, hits


def group_slots(xyz, group):
    """For idx lists group [B, S, K]: (e [B, S, K] float32, vstar [B, S, K]):
    slot 1 of pcm_knn(k = 2) of every group against itself."""
    b, s, k = group.shape
    pts = gather_points(np.asarray(xyz, F32), group).reshape(b * s, k, 3)
    dist, idx = knn_restated(pts, pts, 2)
    return dist[:, :, 1].reshape(b, s, k), idx[:, :, 1].reshape(b, s, k)


def u_values(e):
    """u = sqrtf(e) + 1e-8f in float32, and the float32 root."""
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.asarray(e, F32))
    return (root + F32(1e-8)).astype(F32), root


def uniform_restated(xyz, npoint, nsample, ball_radius, weight, expect_len, groups=None):
    """The contract in float64 over the float32 u values.  Returns a dict:
    loss, groups, hits (None when groups were given), and per scale e, vstar,
    m [B, npoint] and term [B, npoint]."""
    xyz = np.asarray(xyz, F32)
    b = xyz.shape[0]
    hits = None
    if groups is None:
        _, groups, hits = uniform_groups(xyz, npoint, nsample, ball_radius)
    out = {"groups": groups, "hits": hits, "e": [], "vstar": [], "m": [], "term": []}
    loss = 0.0
    L = float(expect_len)
    for q, g in enumerate(groups):
        e, vstar = group_slots(xyz, g)
        u, _ = u_values(e)
        m = u.astype(np.float64).sum(-1) / nsample[q]
        term = (m - L) ** 2 / (L + 1e-8)
        loss += weight[q] * term.sum() / (b * npoint)
        out["e"].append(e)
        out["vstar"].append(vstar)
        out["m"].append(m)
        out["term"].append(term)
    out["loss"] = loss
    return out


def uniform_gradient_f64(xyz, npoint, nsample, weight, expect_len, res):
    """The contract's gradient in float64 over the lists and slots of `res`
    (uniform_restated's dict), with what its float32 error bound needs: (grad
    [B, N, 3], T [B, N] contributions per point, S [B, N, 3] the sum of their
    magnitudes per component)."""
    p32 = np.asarray(xyz, F32)
    p = p32.astype(np.float64)
    b, n, _ = p.shape
    L = float(expect_len)
    grad = np.zeros((b, n, 3))
    mag = np.zeros((b, n, 3))
    count = np.zeros((b, n))
    for q, g in enumerate(res["groups"]):
        e, vstar, m = res["e"][q], res["vstar"][q], res["m"][q]
        _, root = u_values(e)
        c = weight[q] * 2.0 * (m - L) / ((L + 1e-8) * b * npoint * nsample[q])  # [B, S]
        live = (e > 0) & np.isfinite(e)
        for bi in range(b):
            s, t = np.nonzero(live[bi])
            i = g[bi, s, t].astype(np.int64)
            j = g[bi, s, vstar[bi, s, t]].astype(np.int64)
            # the float32 difference is exact in float64 only up to its own rounding: form it in float64
            contrib = c[bi, s][:, None] * (p[bi, i] - p[bi, j]) / root[bi, s, t].astype(np.float64)[:, None]
            np.add.at(grad[bi], i, contrib)
            np.add.at(grad[bi], j, -contrib)
            np.add.at(mag[bi], i, np.abs(contrib))
            np.add.at(mag[bi], j, np.abs(contrib))
            np.add.at(count[bi], i, 1)
            np.add.at(count[bi], j, 1)
    return grad, count, mag


def gradient_bound(count, mag):
    """(T + 6) 2^-23 S per component: per contribution one float32 difference,
    one division, the rounding of the coefficient and one product (2^-24 each),
    and the T - 1 float32 additions of a point's T contributions -- derived,
    not measured."""
    return (count[..., None] + 6.0) * 2.0 ** -23 * mag
