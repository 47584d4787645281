"""The projection loss restated in numpy: the float64 references and the
tolerances of tests/test_silhouette_gpu.py, a float32 restatement of the three
kernels' arithmetic, and the cases that put csrc/silhouette.hip on the edges of
its launch geometry (tests/test_silhouette_edges_cpu.py keeps the cases and the
tolerances honest, tests/test_silhouette_edges_gpu.py runs the device).

Tolerances (none of them fitted to the code under test; derived in
tests/test_silhouette_gpu.py's docstring):
  forward   rtol FWD_RTOL = 1e-4, atol FWD_ATOL = 1e-30 against sil_f64
  backward  |err| <= ((H W + 64) 2^-24 + 2e-5) A + 1e-30 per point and
            coordinate, A the sum over the absolute values of the terms
  loss      (L + 8) 2^-24 mean|term| + 2.4e-7, L = PCM_PROJ_BCE_CHAIN
The float64 restatements start from the float32 co-ordinate map the contract
pins (gx = ((px + 1) H) / 2 in float32) and are float64 from there.

The float32 restatement is the contract's arithmetic with float32 roundings
and a plain order: a factor is exp2((d d) c) with c = float32(-log2e /
(2 sigma_sq)), a cell's sum runs over the points in ascending order, a
gradient's over the columns and then the rows in ascending order, and the BCE
terms are float32 with the summation order include/pcm.h documents (eight
strided elements a thread, a wave's 64 pairwise, four waves in order, the
partials 256 apart in order).  It is not the kernels' order; the CPU test asks
it to stay within a quarter of each tolerance, so that the tolerance leaves
room for another order and for the hardware's exponential.

What the cases meet (csrc/silhouette.hip):
  forward   32 x 32 tiles: grids with one row or column, a partial second,
            third or fourth tile; chunks of 128 points, 16 to a wave.
  backward  bands of 32 rows of G; 1, 2, 4, 8 or 16 slices of eight columns for
            widths up to 8, 16, 32, 64, 128 and P = 64, 64, 64, 32, 16 points a
            workgroup: every slice count with a partial band after a full one,
            widths just past a slice-count edge, n = P - 1, P, P + 1.
  sigma_sq  0.02 (a factor underflows one cell and a half away), 0.5, 2.0 and
            1e4 (every factor close to 1: cells of the size of n).
"""
import collections
import functools

import numpy as np
import torch

F32 = np.float32
FWD_RTOL, FWD_ATOL = 1e-4, 1e-30
U = 2.0 ** -24


WORST = {}  # (kind, grid or count, sigma_sq or gt scale) -> the largest error / tolerance a device test met


def note(kind, where, param, ratio):
    WORST[(kind, where, param)] = max(WORST.get((kind, where, param), 0.0), float(ratio))


# ---------------------------------------------------------------- float64 references


def _pinned(xyz, grid_h, grid_w):
    """(gx, gy) of the contract's float32 co-ordinate map, widened to float64."""
    x = np.asarray(xyz, np.float32)
    gx = ((x[..., 0] + np.float32(1)) * np.float32(grid_h)) / np.float32(2)
    gy = ((x[..., 1] + np.float32(1)) * np.float32(grid_w)) / np.float32(2)
    assert gx.dtype == np.float32
    return gx.astype(np.float64), gy.astype(np.float64)


def _factors(g, cells, sigma_sq):
    d = g[..., None] - np.arange(cells, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(-(d * d) / (2.0 * sigma_sq))
    return d, e


def sil_f64(xyz, grid_h, grid_w, sigma_sq):
    gx, gy = _pinned(xyz, grid_h, grid_w)
    _, ex = _factors(gx, grid_h, sigma_sq)
    _, ey = _factors(gy, grid_w, sigma_sq)
    return np.einsum("bnh,bnw->bhw", ex, ey)


def grad_f64(xyz, G, grid_h, grid_w, sigma_sq):
    """(gradient [B, N, 3], bound term A [B, N, 2]) by float64 autograd of the
    restatement with respect to the pinned grid co-ordinates, times their
    derivative grid / 2; A is the same sum over the absolute values of its terms."""
    gx, gy = _pinned(xyz, grid_h, grid_w)
    tx = torch.from_numpy(gx).requires_grad_()
    ty = torch.from_numpy(gy).requires_grad_()
    ex = torch.exp(-(tx[..., None] - torch.arange(grid_h, dtype=torch.float64)) ** 2 / (2.0 * sigma_sq))
    ey = torch.exp(-(ty[..., None] - torch.arange(grid_w, dtype=torch.float64)) ** 2 / (2.0 * sigma_sq))
    S = torch.einsum("bnh,bnw->bhw", ex, ey)
    G64 = torch.from_numpy(np.asarray(G, np.float64))
    S.backward(G64)
    grad = np.zeros(gx.shape + (3,), np.float64)
    grad[..., 0] = tx.grad.numpy() * (grid_h / 2.0)
    grad[..., 1] = ty.grad.numpy() * (grid_w / 2.0)
    dx, nex = _factors(gx, grid_h, sigma_sq)
    dy, ney = _factors(gy, grid_w, sigma_sq)
    aG = np.abs(np.asarray(G, np.float64))
    A = np.zeros(gx.shape + (2,), np.float64)
    A[..., 0] = np.einsum("bnh,bnw,bhw->bn", np.abs(dx / sigma_sq) * nex, ney, aG) * (grid_h / 2.0)
    A[..., 1] = np.einsum("bnh,bnw,bhw->bn", nex, np.abs(dy / sigma_sq) * ney, aG) * (grid_w / 2.0)
    return grad, A


def _bce_f64(pred, gt, w):
    """(terms, gradient of their mean) in float64 from the float32-pinned a and c."""
    pred = np.asarray(pred, np.float32)
    a = pred + np.float32(1e-8)
    q = (np.float32(1) - pred) - np.float32(1e-8)
    cc = np.abs(q)
    assert a.dtype == np.float32 and q.dtype == np.float32
    a, q, cc, g = a.astype(np.float64), q.astype(np.float64), cc.astype(np.float64), np.asarray(gt, np.float64)
    term = ((-g) * np.log(a)) * w - (1.0 - g) * np.log(cc)
    count = float(np.float32(pred.size))
    grad = (-g * w / a + (1.0 - g) / q) / count
    return term, grad


def backward_bound(grid_h, grid_w, A):
    return ((grid_h * grid_w + 64) * U + 2e-5) * A + 1e-30


def bce_tolerance(term, chain):
    return (chain + 8) * U * np.mean(np.abs(term)) + 2.4e-7


# ---------------------------------------------------------------- float32 restatement


def _factors_f32(g, cells, sigma_sq):
    """(d, exp2((d d) c)) in float32 for g [B, N] float32 -> [B, N, cells]."""
    c = F32(-1.4426950408889634 / (2.0 * float(F32(sigma_sq))))
    d = g[..., None] - np.arange(cells, dtype=F32)
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp2((d * d) * c)
    assert d.dtype == F32 and e.dtype == F32
    return d, e


def _pinned_f32(xyz, grid_h, grid_w):
    x = np.asarray(xyz, F32)
    return ((x[..., 0] + F32(1)) * F32(grid_h)) / F32(2), ((x[..., 1] + F32(1)) * F32(grid_w)) / F32(2)


def sil_f32(xyz, grid_h, grid_w, sigma_sq):
    """The forward in float32: products rounded, the points added in ascending order."""
    gx, gy = _pinned_f32(xyz, grid_h, grid_w)
    _, ex = _factors_f32(gx, grid_h, sigma_sq)
    _, ey = _factors_f32(gy, grid_w, sigma_sq)
    out = np.zeros((ex.shape[0], grid_h, grid_w), F32)
    with np.errstate(under="ignore"):
        for k in range(ex.shape[1]):
            out = out + ex[:, k, :, None] * ey[:, k, None, :]
    assert out.dtype == F32
    return out


def grad_f32(xyz, G, grid_h, grid_w, sigma_sq):
    """The backward in float32 [B, N, 3]: per row the columns in ascending order, then the rows in ascending
    order, times grid / 2; z is 0."""
    gx, gy = _pinned_f32(xyz, grid_h, grid_w)
    dx, ex = _factors_f32(gx, grid_h, sigma_sq)
    dy, ey = _factors_f32(gy, grid_w, sigma_sq)
    inv = F32(1) / F32(sigma_sq)
    with np.errstate(under="ignore"):
        dex, dey = ((-dx) * inv) * ex, ((-dy) * inv) * ey
        G = np.asarray(G, F32)
        b, n = gx.shape
        u = np.zeros((b, n, grid_h), F32)  # sum over w of G[h, w] ey[w]
        v = np.zeros((b, n, grid_h), F32)  # sum over w of G[h, w] dey[w]
        for w in range(grid_w):
            u = u + G[:, None, :, w] * ey[:, :, None, w]
            v = v + G[:, None, :, w] * dey[:, :, None, w]
        ax, ay = np.zeros((b, n), F32), np.zeros((b, n), F32)
        for h in range(grid_h):
            ax = ax + dex[:, :, h] * u[:, :, h]
            ay = ay + ex[:, :, h] * v[:, :, h]
    out = np.zeros((b, n, 3), F32)
    out[..., 0] = (F32(grid_h) / F32(2)) * ax
    out[..., 1] = (F32(grid_w) / F32(2)) * ay
    return out


def bce_terms_f32(pred, gt, w):
    """The 'bce_prob' terms in float32, in the order of loss/proj_loss.py:17-19."""
    pred, gt, w = np.asarray(pred, F32), np.asarray(gt, F32), F32(w)
    a = pred + F32(1e-8)
    cc = np.abs((F32(1) - pred) - F32(1e-8))
    term = ((-gt) * np.log(a)) * w - (F32(1) - gt) * np.log(cc)
    assert term.dtype == F32
    return term


def _workgroup_sums_f32(v):
    """[K, 256] float32, a workgroup's 256 thread sums -> [K]: each wave's 64 pairwise, the four waves in order."""
    w = v.reshape(-1, 4, 64)
    while w.shape[2] > 1:
        w = w[:, :, 0::2] + w[:, :, 1::2]
    s = np.zeros(w.shape[0], F32)
    for k in range(4):
        s = s + w[:, k, 0]
    return s


def bce_loss_f32(term):
    """The mean of the float32 terms in the order include/pcm.h documents for pcm_proj_bce."""
    count = term.size
    nblk = (count + 2047) // 2048
    padded = np.zeros(nblk * 2048, F32)
    padded[:count] = term
    per = padded.reshape(nblk, 8, 256)  # workgroup k, thread t: elements 2048 k + t + 256 j
    s = np.zeros((nblk, 256), F32)
    for j in range(8):
        s = s + per[:, j]
    partials = _workgroup_sums_f32(s)
    if nblk == 1:
        return partials[0] / F32(count)
    trips = (nblk + 255) // 256
    padded = np.zeros(trips * 256, F32)
    padded[:nblk] = partials
    s = np.zeros(256, F32)
    for k in range(trips):  # thread t adds partials t, t + 256, ..
        s = s + padded[256 * k: 256 * k + 256]
    tot = _workgroup_sums_f32(s[None])[0]
    assert tot.dtype == F32
    return tot / F32(count)


# ---------------------------------------------------------------- the cases

Case = collections.namedtuple("Case", "family grid n sigma_sq")
B = 3
N = 300
FAMILIES = ("unit", "wide", "collapsed", "centres", "edge", "duplicates")
FWD_GRIDS = [(1, 1), (1, 128), (128, 1), (8, 17), (17, 8), (31, 33), (33, 31), (32, 65), (65, 32), (63, 127), (97, 64),
             (100, 9), (9, 100), (127, 128), (128, 127)]
BWD_GRIDS = FWD_GRIDS + [(33, 16), (65, 33), (100, 65), (64, 9)]
SIGMA_GRIDS = [(33, 31), (100, 9), (128, 127)]
SIGMAS = (0.02, 0.5, 2.0, 1e4)
FWD_COUNTS = (15, 16, 17, 127, 128, 129, 257)  # the 16-points-a-wave split and the 128-point chunk
FWD_COUNT_GRIDS = [(33, 31), (128, 127)]
BWD_POINTS = {8: 64, 16: 64, 32: 64, 64: 32, 128: 16}  # grid_w -> P, the points of a backward workgroup
BWD_COUNT_HEIGHT = 33


def _grid_cases(grids):
    out = [Case(f, g, N, 0.5) for g in grids for f in FAMILIES]
    out += [Case(f, g, N, s) for g in SIGMA_GRIDS for s in SIGMAS if s != 0.5 for f in FAMILIES]
    return out


FWD_CASES = _grid_cases(FWD_GRIDS) + [Case("unit", g, n, 0.5) for g in FWD_COUNT_GRIDS for n in FWD_COUNTS]
BWD_CASES = _grid_cases(BWD_GRIDS) + [Case("unit", (BWD_COUNT_HEIGHT, w), p + k, 0.5)
                                      for w, p in BWD_POINTS.items() for k in (-1, 0, 1)]


def case_id(c):
    return f"{c.family}-{c.grid[0]}x{c.grid[1]}-n{c.n}-s{c.sigma_sq:g}"


def _on_cell(k, grid):
    """float32 p with ((p + 1) grid) / 2 == k exactly in float32 where one exists within a few neighbours of
    2 k / grid - 1, else the nearest such neighbour."""
    k = np.asarray(k, np.float64)
    best = (2.0 * k / grid - 1.0).astype(F32)
    err = np.abs(((best + F32(1)) * F32(grid)) / F32(2) - k.astype(F32))
    for direction in (-2.0, 2.0):
        p = best.copy()
        for _ in range(4):
            p = np.nextafter(p, F32(direction))
            e = np.abs(((p + F32(1)) * F32(grid)) / F32(2) - k.astype(F32))
            best, err = np.where(e < err, p, best), np.minimum(e, err)
    return best.astype(F32)


@functools.lru_cache(maxsize=None)
def cloud(family, grid, n):
    """[B, n, 3] float32, read-only.  z is random and NaN in every third point: it is never read."""
    h, w = grid
    rng = np.random.default_rng(9000 + 131 * h + 17 * w + n)
    xyz = rng.random((B, n, 3), dtype=F32) * F32(2) - F32(1)
    if family == "wide":  # most terms underflow and whole tiles are 0
        xyz[..., :2] = xyz[..., :2] * F32(3)
    elif family == "collapsed":
        xyz[..., 0], xyz[..., 1] = F32(0.3), F32(-0.6)
    elif family == "centres":  # point k on cell (k mod h, (k div h) mod w): d = 0 terms
        k = np.arange(n)
        xyz[..., 0], xyz[..., 1] = _on_cell(k % h, h), _on_cell((k // h) % w, w)
    elif family == "edge":  # gx = 0 and, from the float32 just below 1, (p + 1) rounding to 2: gx = h
        xyz[..., 0] = np.where(np.arange(n) % 2 == 0, F32(-1), np.nextafter(F32(1), F32(0)))
    elif family == "duplicates":
        half = n // 2
        xyz[:, n - half:] = xyz[:, :half]
    else:
        assert family == "unit"
    xyz[:, ::3, 2] = np.nan
    xyz.setflags(write=False)
    return xyz


def grad_sil(grid, n):
    """The seeded randn G [B, H, W] float32 of a backward case."""
    g = torch.Generator().manual_seed(7000 + 131 * grid[0] + 17 * grid[1] + n)
    return torch.randn(B, grid[0], grid[1], generator=g).numpy()


def bwd_slices(grid_w):
    """Slices of eight columns per point (csrc/silhouette.hip sil_bwd_slices) and the points of a workgroup."""
    sl = 1
    while sl * 8 < grid_w:
        sl *= 2
    return sl, min(256 // sl, 64)


# ---------------------------------------------------------------- pcm_proj_bce cases

BCE_COUNTS = (1, 63, 4097, 32 * 64 * 64)
BCE_NEW_COUNTS = (2047, 2048, 2049, 524288, 524289, 2048 * 257, 1048576)
BCE_GT_SCALES = (1.0, 3.0)  # gt = rand: probabilities; gt = rand * 3: silhouettes, above 1 where points overlap


def bce_inputs(count, gt_scale):
    """(pred, gt) float32 torch tensors of tests/test_silhouette_gpu.py's seed: pred = rand * 3."""
    g = torch.Generator().manual_seed(41)
    pred = torch.rand(count, generator=g) * 3
    gt = torch.rand(count, generator=g)
    return pred, (gt * gt_scale if gt_scale != 1.0 else gt)


def bce_edge_vector():
    """pred in {0, 1e-30, 2^-24, the float32 just below 1, 1, the one just above 1, 2.5} crossed with gt in
    {0, 1, 0.5, 2}: 28 elements.  At pred = 1 and at the float32 just below it |(1 - pred) - 1e-8| is 1e-8 and
    5.96e-8 - 1e-8 = 4.96e-8; at pred = 0 and 1e-30 a = 1e-8."""
    one = F32(1)
    preds = np.array([0.0, 1e-30, 2.0 ** -24, np.nextafter(one, F32(0)), 1.0, np.nextafter(one, F32(2)), 2.5], F32)
    gts = np.array([0.0, 1.0, 0.5, 2.0], F32)
    return np.repeat(preds, len(gts)), np.tile(gts, len(preds))
