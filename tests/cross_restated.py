"""Numpy restatement of the cross Chamfer matrix (include/pcm.h,
pcm_chamfer_cross) and of utils/set_metrics.py -- a helper, not a test.

The per-point distances of a pair of clouds come from the CPU oracle's
chamfer_forward (bit-exact with the HIP forward by the existing suite); an entry
is np.float32(math.fsum(d as float64) / n): the correctly rounded sum, divided
and rounded once.  The product adds in float64 in its own fixed order, which
may differ from the exact sum by a few float64 roundings (relative 1e-13 at
16384 terms) -- so an entry is never more than 1 float32 ulp off, and is off at
all only when the quotient lies within 1e-13 of a rounding boundary, about one
entry in a million.  MAX_INEXACT_SHARE (0.1 %) is the cap both test files hold.

The set metrics are written as plain loops; the first minimum wins every tie.
"""
import functools
import math

import numpy as np

F32 = np.float32
MAX_ULP = 1
MAX_INEXACT_SHARE = 1e-3

# launch geometry of csrc/chamfer_cross.hip, as pcm_hip exports it (tests/test_cross_cpu.py asserts they agree)
QUERIES, TILE, J, MIN_BLOCKS = 1024, 1024, 8, 256

# (s, r, n, m): the issue's shapes ...
FIXED_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 5), (3, 2, 7, 300), (2, 3, 64, 65), (4, 5, 1024, 1024), (2, 2, 2049, 2047),
                (1, 2, 16384, 100), (2, 1, 16384, 16384)]
# ... and one on each side of every geometry constant.  QUERIES and TILE are both 1024 and the two directions
# swap the clouds' roles, so (1023, 1025) has a query block one short with a one-point second tile in direction 1,
# and a one-query second block (the finalise launch) over a tile one short in direction 2; (1024, 1025) sits on
# the single-record / finalise split itself.  r = J - 1, J, J + 1, 2 J + 1 at s = 144, where the grid is large
# enough for runs of J clouds; (40, 9) takes runs of 2 and (3, 9) runs of 1 (EDGE_RUNS, asserted on the library).
EDGE_SHAPES = [(1, 2, QUERIES - 1, TILE + 1), (2, 1, QUERIES + 1, TILE - 1), (2, 2, QUERIES, TILE + 1),
               (144, J - 1, 5, 6), (144, J, 5, 6), (144, J + 1, 5, 6), (144, 2 * J + 1, 5, 6),
               (40, J + 1, 3, 4), (3, J + 1, 7, 5)]
EDGE_RUNS = {(144, J - 1, 5, 6): J, (144, J, 5, 6): J, (144, J + 1, 5, 6): J, (144, 2 * J + 1, 5, 6): J,
             (40, J + 1, 3, 4): 2, (3, J + 1, 7, 5): 1}
SHAPES = FIXED_SHAPES + EDGE_SHAPES
# what a CPU test can afford
SMALL_SHAPES = [sh for sh in SHAPES if sh[0] * sh[1] * sh[2] * sh[3] <= 1 << 23]


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def make_sets(s, r, n, m, seed=None):
    """Two seeded sets of uniform float32 clouds, x [s, n, 3] and y [r, m, 3], read-only."""
    rng = np.random.default_rng(9100 + 131 * s + 17 * r + 7 * n + m if seed is None else seed)
    x, y = rng.random((s, n, 3), dtype=F32), rng.random((r, m, 3), dtype=F32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _oracle():
    import oracle as O
    O.build()
    return O


def pair_distances(x, y):
    """(d1 [s, r, n], d2 [s, r, m]) float32: the oracle's nearest squared distances of every pair (x[i], y[j])."""
    O = _oracle()
    s, n = x.shape[:2]
    r, m = y.shape[:2]
    d1, d2 = np.empty((s, r, n), F32), np.empty((s, r, m), F32)
    for j in range(r):
        yj = np.ascontiguousarray(np.broadcast_to(y[j], (s, m, 3)), dtype=F32)
        a, b, _, _ = O.chamfer_forward(np.ascontiguousarray(x, dtype=F32), yj)
        d1[:, j], d2[:, j] = a, b
    return d1, d2


def mean_exact(d):
    """np.float32(fsum(d) / len(d)) over the last axis."""
    flat = d.reshape(-1, d.shape[-1]).astype(np.float64)
    out = np.array([F32(math.fsum(row) / d.shape[-1]) for row in flat], dtype=F32)
    return out.reshape(d.shape[:-1])


def cross_means(x, y):
    """(mean12, mean21), both [s, r] float32, of the restatement."""
    d1, d2 = pair_distances(x, y)
    return mean_exact(d1), mean_exact(d2)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(x, y, mean12, mean21) of a shape of SHAPES, computed once, read-only."""
    x, y = make_sets(*shape)
    m12, m21 = cross_means(x, y)
    m12.setflags(write=False)
    m21.setflags(write=False)
    return x, y, m12, m21


def ulp_distance(a, b):
    """Element-wise distance in float32 units in the last place (NaN or sign mismatch: a huge number)."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    out = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) | np.isnan(b), np.int64(1) << 40, out)


class Tally:
    """Entries compared in a test file and how many were not bit-equal."""

    def __init__(self):
        self.entries = 0
        self.inexact = 0

    def check(self, got, want, what=""):
        u = ulp_distance(got, want)
        self.entries += u.size
        self.inexact += int((u != 0).sum())
        worst = int(u.max()) if u.size else 0
        print(f"{what}: {u.size} entries, {int((u != 0).sum())} not bit-equal, largest distance {worst} ulp")
        assert worst <= MAX_ULP, (what, worst)

    def share(self):
        return self.inexact / max(self.entries, 1)


# ---------------------------------------------------------------------------
# the set metrics, as loops
# ---------------------------------------------------------------------------
def _first_min(row):
    best, at = None, -1
    for k, v in enumerate(row):
        if best is None or v < best:
            best, at = v, k
    return at, best


def nearest_shape(cd):
    """(idx [S], cd [S]) of the matrix cd [S, R]: every row's first minimum."""
    pairs = [_first_min(row) for row in np.asarray(cd)]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.asarray(cd).dtype)


def mmd_cov(cd):
    cd = np.asarray(cd)
    s, r = cd.shape
    mmd = math.fsum(float(_first_min(cd[:, j])[1]) for j in range(r)) / r
    chosen = set(_first_min(cd[i])[0] for i in range(s))
    return mmd, len(chosen) / r


def one_nna(cd_ss, cd_sr, cd_rr):
    cd_ss, cd_sr, cd_rr = np.asarray(cd_ss), np.asarray(cd_sr), np.asarray(cd_rr)
    s, r = cd_sr.shape
    right = 0
    for a in range(s + r):
        row = []
        for b in range(s + r):
            if a == b:
                row.append(math.inf)
            elif a < s:
                row.append(cd_ss[a, b] if b < s else cd_sr[a, b - s])
            else:
                row.append(cd_sr[b, a - s] if b < s else cd_rr[a - s, b - s])
        nearest = _first_min(row)[0]
        right += int((nearest >= s) == (a >= s))
    return right / (s + r)
