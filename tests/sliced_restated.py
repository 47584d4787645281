"""numpy restatement of pcm_sliced_wasserstein_loss's contract (include/pcm.h):
the float32 projections bit for bit, the pinned total order as a lexsort, and
the loss, the slices and both gradients in float64 over those orders.  Test
infrastructure only: the GPU tests compare the kernels with it, the CPU tests
check it against brute-force identities.

Projection.  p = fmaf(tz, z, fmaf(ty, y, tx * x)): the product in float32, each
fused step in float64 (a product of two float32 is exact there) and rounded
once to float32, as knn_restated.sqd_pinned does.  A NaN operand comes through
with its sign and payload (quieted), which is what the device's instructions
and numpy's both do; a NaN made from finite or infinite operands (0 * inf,
inf - inf) has no pinned bits and the tests make none.

Order.  key = bits ^ 0xFFFFFFFF if the sign bit is set, else bits | 0x80000000;
order = np.lexsort((index, key)).  The kernels must EQUAL it.

Matching.  On the axis [0, n m) rank r of x owns [r m, (r + 1) m) and rank s of
y owns [s n, (s + 1) n); the union of both sets of breakpoints cuts the axis
into n + m - gcd(n, m) segments, each inside exactly one (r, s) with the
contract's weight w_rs = min((r+1) m, (s+1) n) - max(r m, s n) as its length.
``pairs(n, m)`` lists them; test_sliced_cpu.py checks the list against the
contract's interval formula and against a brute quantile integration.

Error bounds (what a float32 output may differ from this float64 value by).
They are worst-case bounds of an evaluation in float32 with u = 2^-24, from the
term counts and magnitudes, so that they hold for ANY order of the sums and do
not presume the kernels' double accumulators (which sit far inside them):
  slice.  K = n + m - gcd terms w d^2 >= 0 with d = fl(a - b): the difference,
    the square, the weight are (1 + u)^4 a term, a sum of K non-negative terms
    in any order is within (K - 1) u of itself, the division by n m one more:
      |err slice| <= (K + 6) u slice.
  loss.  The mean of l non-negative slices adds (l - 1) u and the division:
      |err loss| <= (K + 6 + l + 1) u loss.
  gradient.  A point's coefficient c = (2 / (n m)) sum_s w_rs (a_r - b_s) has
    k_r <= ceil(other / own) + 1 terms of magnitude <= w_rs D, D the largest
    matched |a_r - b_s| of the element, and sum_s w_rs = other, so |c| <= 2 D /
    own and |err c| <= (k_r + 4) u 2 D / own.  The gradient (1/l) sum_li
    theta_li c_li adds a product, l - 1 additions and the division, each
    against sum |theta| |c| <= l T 2 D / own with T the largest |component| of
    a direction:
      |err grad| <= (ceil(other / own) + 5 + l + 1) u T 2 D / own.
``bounds`` returns SAFETY = 4 times these worst cases: with one or two terms a
float32 evaluation can come close to its worst case (n = m = 1: (a - b)^2 alone
is up to 4 u out), and test_sliced_cpu.py asks that such an evaluation stay
within a QUARTER of every bound -- which four times the worst case grants by
construction for any order of evaluation.
SW(x, x) has every d = 0 exactly: all three bounds are 0 there and so are the
kernels' outputs.
"""
import math

import numpy as np

U32 = 2.0 ** -24
SAFETY = 4.0
MAX_POINTS, MAX_DIRS, FUSED_MAX_POINTS = 16384, 1024, 2048

# the GPU test's shapes (n, m), direction counts and batch sizes
SHAPES = [(1, 1), (1, 9), (7, 5), (64, 64), (256, 256), (1000, 1000), (1024, 1024), (1025, 1025), (1000, 333),
          (128, 1024), (1024, 256)]
DIRS = [1, 3, 64, 65]
BATCHES = [1, 3]
LARGE = [(16384, 16384), (16384, 4096)]  # at b = 1, l = 4


def cases():
    """(b, n, m, l) of the GPU comparison: every shape with two (l, b) pairs,
    rotated so that every l in DIRS and both batch sizes meet small, ragged and
    1024-point shapes."""
    combos = [(l, b) for l in DIRS for b in BATCHES]
    out = []
    for k, (n, m) in enumerate(SHAPES):
        for l, b in (combos[(2 * k) % 8], combos[(2 * k + 5) % 8]):
            out.append((b, n, m, l))
    return out


def make_clouds(b, n, m, seed=0):
    """x uniform in the unit cube, y uniform in a smaller shifted box: float32."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * m + b)
    x = rng.random((b, n, 3), dtype=np.float32)
    y = (np.float32(0.7) * rng.random((b, m, 3), dtype=np.float32) + np.float32(0.25)).astype(np.float32)
    return x, y


def make_dirs(l, seed=0):
    """l random unit directions, float32 (normalised in float64, rounded once)."""
    rng = np.random.default_rng(77 + 13 * seed + l)
    d = rng.standard_normal((l, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# axis-aligned directions and directions whose components are multiples of 1/8: with lattice coordinates
# every product and sum is exact, so projections tie exactly (256 points have 8 distinct ones on an axis)
LATTICE_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.125, 0.375, -0.625], [-1, 0.5, 0.25],
                         [0.875, -0.125, 0.5], [0.25, 0.25, 0.25]], np.float32)
# signed zeros in the directions too: 0 * negative = -0.0, and -0.0 survives a sum only with another -0.0
ZERO_DIRS = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, -0.0, 0.0], [0.5, 0.5, -0.0]], np.float32)


def make_lattice(b, n, m, seed=0):
    """Coordinates on the 1/8 lattice of the unit cube: float32, many exact ties."""
    rng = np.random.default_rng(500 + seed + n + 2 * m + b)
    return ((rng.integers(0, 8, (b, n, 3)) / 8).astype(np.float32),
            (rng.integers(0, 8, (b, m, 3)) / 8).astype(np.float32))


def make_zeros(b, n, m, seed=0):
    """Coordinates drawn from -0.0, +0.0, -0.5, 0.5 (half of them zeros of either sign)."""
    rng = np.random.default_rng(900 + seed + n + 2 * m + b)
    vals = np.array([-0.0, 0.0, -0.0, 0.0, -0.5, 0.5], np.float32)
    return vals[rng.integers(0, 6, (b, n, 3))], vals[rng.integers(0, 6, (b, m, 3))]


def make_duplicates(b, n, m, seed=0):
    """make_clouds with every point present three or four times over, shuffled."""
    rng = np.random.default_rng(1300 + seed + n + 2 * m + b)
    x, y = make_clouds(b, -(-n // 4), -(-m // 3), seed)
    x = np.repeat(x, 4, axis=1)[:, rng.permutation(4 * x.shape[1])[:n]]
    y = np.repeat(y, 3, axis=1)[:, rng.permutation(3 * y.shape[1])[:m]]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def project(pts, dirs, fused=True):
    """[l, n] float32 projections of pts [n, 3] on dirs [l, 3], pinned.
    fused=False: every product and sum rounded to float32 (a modelled defect)."""
    pts, dirs = np.asarray(pts, np.float32), np.asarray(dirs, np.float32)
    x, y, z = pts[None, :, 0], pts[None, :, 1], pts[None, :, 2]
    tx, ty, tz = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (tx * x).astype(np.float32)
        if not fused:
            t = (t + (ty * y).astype(np.float32)).astype(np.float32)
            return (t + (tz * z).astype(np.float32)).astype(np.float32)
        t = (ty.astype(np.float64) * y + t).astype(np.float32)
        return (tz.astype(np.float64) * z + t).astype(np.float32)


def keys(p):
    u = np.ascontiguousarray(p, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), u ^ np.uint32(0xFFFFFFFF), u | np.uint32(0x80000000))


def orders(p, descending_ties=False, merge_zeros=False):
    """[l, n] int32: the point of every rank.  The two flags model defects."""
    k = keys(p)
    if merge_zeros:  # -0.0 (key 0x7FFFFFFF) treated as +0.0 (key 0x80000000)
        k = np.where(k == np.uint32(0x7FFFFFFF), np.uint32(0x80000000), k)
    idx = np.arange(p.shape[1])
    tie = -idx if descending_ties else idx
    return np.stack([np.lexsort((tie, row)) for row in k]).astype(np.int32)


_pairs_cache = {}


def pairs(n, m):
    """(r, s, w) int64 arrays of the n + m - gcd(n, m) overlapping rank pairs, ascending."""
    if (n, m) not in _pairs_cache:
        cuts = np.union1d(np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n)
        lo, hi = cuts[:-1], cuts[1:]
        _pairs_cache[(n, m)] = (lo // m, lo // n, hi - lo)
    return _pairs_cache[(n, m)]


def pairs_by_formula(n, m, floor_defect=False):
    """The same list straight from the contract's interval formula (a Python loop).
    floor_defect: the upper overlap rank taken with floor instead of ceil."""
    R, S, W = [], [], []
    for r in range(n):
        lo = (r * m) // n
        hi = ((r + 1) * m) // n - 1 if floor_defect else -((-(r + 1) * m) // n) - 1
        for s in range(lo, hi + 1):
            R.append(r)
            S.append(s)
            W.append(min((r + 1) * m, (s + 1) * n) - max(r * m, s * n))
    return np.array(R, np.int64), np.array(S, np.int64), np.array(W, np.int64)


def sliced_one(x, y, dirs, dtype=np.float64, rsw=None, fused=True, order_flags=None, drop_last=False):
    """One element: dict(loss, slices [l], gx [n, 3], gy [m, 3], order1 [l, n],
    order2 [l, m], D) evaluated in ``dtype`` over the pinned projections and
    orders.  rsw / fused / order_flags / drop_last model defects."""
    x, y, dirs = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(dirs, np.float32)
    n, m, l = len(x), len(y), len(dirs)
    p1, p2 = project(x, dirs, fused), project(y, dirs, fused)
    o1, o2 = orders(p1, **(order_flags or {})), orders(p2, **(order_flags or {}))
    r, s, w = pairs(n, m) if rsw is None else rsw
    wt = w.astype(dtype)
    nm = dtype(n) * dtype(m)
    use = l - 1 if drop_last else l
    slices = np.zeros(l, dtype)
    gx, gy = np.zeros((n, 3), dtype), np.zeros((m, 3), dtype)
    D = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for li in range(use):
            a, b = p1[li, o1[li]].astype(dtype), p2[li, o2[li]].astype(dtype)
            d = a[r] - b[s]
            if len(d) and np.isfinite(d).all():
                D = max(D, float(np.abs(d).max()))
            wd = wt * d
            slices[li] = (wd * d).sum(dtype=dtype) / nm
            c1 = (dtype(2) / nm) * np.bincount(r, wd, n).astype(dtype)
            c2 = (dtype(2) / nm) * np.bincount(s, -wd, m).astype(dtype)
            if dtype == np.float32:  # bincount adds in float64: model the rounded coefficient
                c1, c2 = c1.astype(np.float32), c2.astype(np.float32)
            th = dirs[li].astype(dtype)
            gx[o1[li]] += c1[:, None] * th[None, :]
            gy[o2[li]] += c2[:, None] * th[None, :]
        div = dtype(max(use, 1))
        loss = slices[:use].sum(dtype=dtype) / div if use else dtype(0)
        gx, gy = gx / div, gy / div
    return dict(loss=loss, slices=slices, gx=gx, gy=gy, order1=o1, order2=o2, D=D)


def bounds(n, m, l, res, dirs):
    """(loss, slices [l], grad x, grad y) bounds of one element (see the module text)."""
    K = n + m - math.gcd(n, m)
    T = float(np.abs(np.asarray(dirs, np.float64)).max())
    loss = (K + 6 + l + 1) * U32 * abs(float(res["loss"]))
    slices = (K + 6) * U32 * np.abs(np.asarray(res["slices"], np.float64))
    gx = (-(-m // n) + 5 + l + 1) * U32 * T * 2.0 * res["D"] / n
    gy = (-(-n // m) + 5 + l + 1) * U32 * T * 2.0 * res["D"] / m
    return SAFETY * loss, SAFETY * slices, SAFETY * gx, SAFETY * gy


_restated_cache = {}


def restated(b, n, m, l, seed=0):
    """(x, y, dirs, [per-element result dicts]) for make_clouds / make_dirs inputs,
    computed once and shared (treat as read-only)."""
    key = (b, n, m, l, seed)
    if key not in _restated_cache:
        x, y = make_clouds(b, n, m, seed)
        dirs = make_dirs(l, seed)
        _restated_cache[key] = (x, y, dirs, [sliced_one(x[i], y[i], dirs) for i in range(b)])
    return _restated_cache[key]
