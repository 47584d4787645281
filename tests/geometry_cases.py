"""Inputs outside the unit cube and on degenerate geometry for the newer losses
(kNN / repulsion, FPS, ball query, the uniform loss, the kernel norms, Sinkhorn,
sliced Wasserstein, DCD) and for the ninth op, the one-pass Chamfer evaluation
behind fscore (csrc/chamfer_eval.hip).

Shared by tests/test_geometry_cpu.py (which keeps the inputs, the restatements
and the bounds honest on these clouds) and tests/test_geometry_gpu.py (the HIP
kernels against the restatements).  Everything is seeded numpy, so both see
the same bits.

A family is a transform of a base pair (x, y) that comes from the op's own
make_clouds / make_cloud (kNN and the ball query have none: seeded uniform
clouds, the ball query's centres drawn over [-0.2, 1.2)^3 as its own test
does), so every shape, seed and edge-of-tile property of the per-op suites is
kept.  Ops that take one cloud use x.  What each family moves:
  * centred (both - 0.5): negative coordinates -- the sign branch of
    csrc/sliced.hip's key (bits ^ 0xFFFFFFFF), signed projections, dx of
    either sign in every fmaf chain.
  * generator (x 3 - 1.5, y unchanged): the training call's ranges; d2 up to
    27 in csrc/sinkhorn.hip's fmaf(d2, c, h) and csrc/kernel_loss.hip's
    exponent, a cross term that dominates the own terms.
  * scale_1e3, scale_1e-3 (both times s; blur, diameter, radii, expect_len
    times s, the repulsion h times s^2): the magnitude of d2 against the
    float constants c = -log2e / (2 eps) and s = log2e / eps of the Sinkhorn
    step, sc.r2 = radius * radius of csrc/grouping.hip, the potentials' size.
  * offset_1000 (both + 1000): cancellation in p[k] - p[far]; coordinates are
    quantised to 2^-14 = 6.1e-5, so every difference is exact, dx = 0
    between distinct points is common and `d < ld[W - 1]` (knn.hip), `d <
    sc.r2[q]` (grouping.hip) and `d < run` (sampling.hip) compare sums of exact squares
    with exact ties among a query's candidates (in three dimensions no two
    distinct points coincide: d = 0 between distinct indices comes from
    duplicates, collapsed and identical).
  * plane (z = 0.5), line (y = z = 0.25): runs of equal (key << 32) | index
    composites in csrc/sliced.hip ordered by the index half alone; coplanar
    and collinear neighbours; 1-D transport.
  * collapsed (x[:] = (0.3, 0.6, 0.9)): every argmin of csrc/dcd.hip's count
    pass is index 0 (one count = the whole other cloud, the rest 0); all-zero
    own distances (the r = 0 rule of kernel_loss.hip, FPS minima all 0).
  * identical (y = x.copy(), n = m: the first cloud twice at the op's first
    shape): losses of exactly 0 and zero gradients where the contract says so.
  * duplicates (the second half of each cloud repeats the first): lowest-index
    ties between bit-equal points in every argmin, list insert and sort.
  * bimodal (x[: n // 2] and y[m // 2 :] + (1000, 0, 0)): exponents that
    underflow (exp2 of -1e7 in kernel_loss.hip); its Sinkhorn schedule has 17
    entries from eps_0 = 1e6, but Sinkhorn leaves the family out (see
    FAMILIES below: no tolerance holds both of its conditions there).
  * far_point (y[:, 7] = (30, -30, 30)): one outlier stretching the diameter;
    the one DCD term with alpha d far above 16000.
  * scale_2e5 (FPS only): squared distances above kFpsFar = 1e10f, so running
    minima stay saturated and the next seed is the lowest saturated index.
  * scale_1e-20 (FPS, ball query, F-score): every squared distance is a float32
    subnormal, which `d < run`, the wave maximum (sampling.hip: "float32
    denormals preserved"), `d < sc.r2[q]` and, in chamfer_eval.hip, the packed
    fp32 scan (pcm_sqd2), its running minimum and the `d < th.v[t]` ballots
    must keep; the F-score thresholds go with s^2, so the first three are
    subnormal themselves (1e-44, 1e-43, 1e-42).
  * offset_duplicates (duplicates, then + 1000; kNN, repulsion, FPS, the
    ball query and F-score -- not in the issue's table): what offset_1000 alone cannot
    have in three dimensions, at coordinate 1000: d = 0 between distinct
    indices (the self search's slot 1, FPS minima) and exact ties inside a
    list.
Families an op does not take: identical and far_point change only y and go to
the two-cloud ops.  For the ball query x is the centres and y the cloud they
search: collapsed gives 65 equal centres (every ball the same list), identical
searches the centres themselves, so every ball holds its own centre at d = 0
and none is empty (the one family exempt from the three-kinds assertion).
The F-score op takes seeded uniform clouds as kNN does; its shapes take 2 queries
per lane (eval_qpt), the second with one direction exactly on the 2048-candidate
LDS tile and the other one below it.  Its thresholds are FSCORE_THS times s^2
rounded to float32, its reference the oracle's chamfer_forward.
Non-finite coordinates (every op has a test for them) and magnitudes at which
a float32 squared distance overflows are out of scope.
"""
import collections
import functools
import math

import numpy as np

import dcd_restated as D
import kernel_loss_restated as K
import sinkhorn_restated as S
import sliced_restated as SL
import uniform_restated as U

F32 = np.float32
Case = collections.namedtuple("Case", "op family shape x y s")


def _f32(*v):
    return np.array(v, dtype=F32)


def _scaled(s):
    return lambda x, y: ((x * F32(s)).astype(F32), (y * F32(s)).astype(F32))


def _unit(x, y):
    return x, y


def _centred(x, y):
    return x - F32(0.5), y - F32(0.5)


def _generator(x, y):
    return (x * F32(3) - F32(1.5)).astype(F32), y


def _offset(x, y):
    return x + _f32(1000, 1000, 1000), y + _f32(1000, 1000, 1000)


def _plane(x, y):
    x[..., 2] = 0.5
    y[..., 2] = 0.5
    return x, y


def _line(x, y):
    x[..., 1:] = 0.25
    y[..., 1:] = 0.25
    return x, y


def _collapsed(x, y):
    x[:] = _f32(0.3, 0.6, 0.9)
    return x, y


def _identical(x, y):
    assert x.shape == y.shape
    return x, x.copy()


def _duplicates(x, y):
    for c in (x, y):
        half = c.shape[1] // 2
        if half:
            c[:, c.shape[1] - half:] = c[:, :half]
    return x, y


def _bimodal(x, y):
    x[:, : x.shape[1] // 2] += _f32(1000, 0, 0)
    y[:, y.shape[1] // 2:] += _f32(1000, 0, 0)
    return x, y


def _far_point(x, y):
    assert y.shape[1] >= 8
    y[:, 7] = _f32(30, -30, 30)
    return x, y


SCALES = {"scale_1e3": 1e3, "scale_1e-3": 1e-3, "scale_2e5": 2e5, "scale_1e-20": 1e-20, "scale_1024": 1024.0}
TRANSFORMS = {"unit": _unit, "centred": _centred, "generator": _generator, "offset_1000": _offset, "plane": _plane,
              "line": _line, "collapsed": _collapsed, "identical": _identical, "duplicates": _duplicates,
              "bimodal": _bimodal, "far_point": _far_point}
TRANSFORMS.update({name: _scaled(s) for name, s in SCALES.items()})
TRANSFORMS["offset_duplicates"] = lambda x, y: _offset(*_duplicates(x, y))

GENERAL = ("centred", "generator", "scale_1e3", "scale_1e-3", "offset_1000", "plane", "line", "collapsed", "identical",
           "duplicates", "bimodal", "far_point")
ONE_CLOUD = tuple(f for f in GENERAL if f not in ("identical", "far_point"))
FAMILIES = {
    "knn": GENERAL + ("offset_duplicates",), "repulsion": ONE_CLOUD + ("offset_duplicates",),
    "fps": ONE_CLOUD + ("scale_2e5", "scale_1e-20", "offset_duplicates"),
    "ball": GENERAL + ("scale_1e-20", "offset_duplicates"),
    "uniform": ONE_CLOUD, "kernel": GENERAL, "sinkhorn": tuple(f for f in GENERAL if f != "bimodal"),
    "sliced": GENERAL, "dcd": GENERAL, "fscore": GENERAL + ("scale_1e-20", "offset_duplicates"),
}
# Sinkhorn leaves out `bimodal`: its diameter is 1001 while the transport is between unit-size halves, so the
# tolerances scaled by D (0.33 on a loss of 14, 0.058 on n |grad| of 0.8) are wider than what a left-out schedule
# entry moves (1.3 to 3.1 gradient tolerances), and four times the float32 restatement's own error (0.46 of the
# scaled gradient tolerance) is still wider than a tenth of it: no tolerance holds both conditions
# (tests/test_geometry_cpu.py asserts this).
# `far_point` takes four times the float32 restatement's own error as its tolerances although that error is
# within a quarter of the scaled ones: at (300, 1025) a left-out last schedule entry (0.0025 after 0.00263)
# moves n |grad| by 9.94 scaled tolerances, short of the ten that condition (b) demands; the narrower tolerance
# (0.34 of the scaled gradient one) holds both.
SINKHORN_OWN_ERROR = ("far_point",)
# "unit" (the base pair itself) and "scale_1024" are not families of the comparison: the power-of-two check uses them

# (b, n, m) -- for fps (b, n, npoint), for the ball query (b, centres, points), for sliced (b, n, m, l)
SHAPES = {
    "knn": [(2, 300, 1025)], "repulsion": [(2, 300, 300)], "fps": [(2, 300, 20), (2, 1025, 33)],
    "ball": [(2, 65, 257)], "uniform": [(2, 300, 300)], "kernel": [(2, 257, 255), (2, 300, 1025)],
    "sinkhorn": [(2, 127, 128), (2, 300, 1025)], "sliced": [(2, 1000, 333, 65), (2, 1025, 1025, 3)],
    "dcd": [(2, 1000, 333), (2, 1025, 1023)], "fscore": [(2, 300, 1025), (2, 2048, 2047)],
}
FSCORE_WIDE_SHAPE = (64, 1030, 700)  # the 4-queries-per-lane kernel: `centred` and `offset_1000` only
FSCORE_THS = (1e-4, 1e-3, 1e-2, 1.0, 30.0)
KNN_KS = (5, 20)
REPULSION_H = 0.01
BALL_NSAMPLE, BALL_RADII = 12, (0.05, 0.3)
UNIFORM_PERCENTAGE = [0.04, 0.08, 0.2]  # tests/test_uniform_gpu.py's SMALL
KERNEL_BLUR = 0.2
SINKHORN_BLUR, SINKHORN_SCALING = 0.05, 0.5
DCD_LAMBDAS = (1.0, 0.5)


def _base(op, b, n, m):
    if op in ("knn", "repulsion", "fscore"):
        rng = np.random.default_rng(4100 + 7 * n + m)
        return rng.random((b, n, 3), dtype=F32), rng.random((b, m, 3), dtype=F32)
    if op == "fps":
        return U.make_cloud("cube", b, n, 100 + n), U.make_cloud("cube", b, n, 200 + n)
    if op == "uniform":
        return U.make_cloud("cube", b, n, 100 + n), U.make_cloud("cube", b, m, 200 + m)
    if op == "ball":  # x: the centres, drawn on their own over [-0.2, 1.2)^3; y: the cloud they search
        rng = np.random.default_rng(7000 + m)
        y = rng.random((b, m, 3), dtype=F32)
        return (rng.random((b, n, 3), dtype=F32) * F32(1.4) - F32(0.2)).astype(F32), y
    if op in ("kernel", "sinkhorn"):
        return K.make_clouds(b, n, m)
    if op == "sliced":
        return SL.make_clouds(b, n, m)
    assert op == "dcd"
    return D.make_clouds(b, n, m)


def entries(op):
    """(family, shape) of the comparison: every family of the op at every shape; `identical` at the first only."""
    return [(f, s) for s in SHAPES[op] for f in FAMILIES[op] if f != "identical" or s == SHAPES[op][0]]


def entry_id(entry):
    return f"{entry[0]}-" + "x".join(str(v) for v in entry[1])


@functools.lru_cache(maxsize=None)
def case(op, family, shape):
    """The family's two float32 clouds (read-only) and its scale s."""
    b, n = shape[0], shape[1]
    m = n if family == "identical" or op == "fps" else shape[2]
    x, y = _base(op, b, n, m)
    x, y = TRANSFORMS[family](np.array(x, F32), np.array(y, F32))
    x, y = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(y, dtype=F32)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return Case(op, family, shape, x, y, SCALES.get(family, 1.0))


def other_family(op, family):
    """The family whose call goes through the cached workspace between a case's two runs: 1e3-scale data."""
    return "scale_1e3" if family != "scale_1e3" else "centred"


def diameter(c):
    """The Sinkhorn call's diameter: the unit cube's diagonal times s for a scaled cloud, else the float32
    bounding-box diagonal of both clouds."""
    if c.family in SCALES:
        return float(F32(S.DIAMETER * c.s))
    return float(F32(K.diameter(c.x, c.y)))


def uniform_params(c):
    """uniform_restated.uniform_params with the radii and expect_len carried along with the cloud's scale."""
    npoint, nsample, radius, weight, L = U.uniform_params(c.shape[1], UNIFORM_PERCENTAGE)
    return npoint, nsample, [r * c.s for r in radius], weight, L * c.s


# ---------------------------------------------------------------------------
# references shared by the CPU and the GPU test, computed once
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def knn_reference(family, shape=SHAPES["knn"][0]):
    c = case("knn", family, shape)
    return U.knn_restated(c.x, c.y, max(KNN_KS))


@functools.lru_cache(maxsize=None)
def fps_reference(family, shape):
    return U.fps_restated(case("fps", family, shape).x, shape[2])


def fps_first_distances(x):
    """The first iteration's pinned float32 distances to point 0, [B, N]."""
    d = x - x[:, :1]
    return U.sqd_pinned(d[..., 0], d[..., 1], d[..., 2])


@functools.lru_cache(maxsize=None)
def ball_reference(family, radius_index, shape=SHAPES["ball"][0]):
    c = case("ball", family, shape)
    return U.ball_query_restated(c.y, c.x, BALL_RADII[radius_index] * c.s, BALL_NSAMPLE)


@functools.lru_cache(maxsize=None)
def uniform_reference(family, shape=SHAPES["uniform"][0]):
    c = case("uniform", family, shape)
    npoint, nsample, radius, weight, L = uniform_params(c)
    res = U.uniform_restated(c.x, npoint, nsample, radius, weight, L)
    return res, U.uniform_gradient_f64(c.x, npoint, nsample, weight, L, res)


@functools.lru_cache(maxsize=None)
def kernel_reference(family, shape, kernel):
    c = case("kernel", family, shape)
    res = [K.restated_one(c.x[i], c.y[i], kernel, KERNEL_BLUR * c.s) for i in range(shape[0])]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def sinkhorn_scaled_tolerances(diam):
    """sinkhorn_restated's tolerances carried to a problem of diameter D: loss_out and the potentials go like
    D^2, n |grad| like D; they were set at the unit cube's diagonal."""
    q = diam / S.DIAMETER
    return S.TOL_LOSS * q * q, S.TOL_GRAD * q, S.TOL_POT * q * q


@functools.lru_cache(maxsize=None)
def sinkhorn_reference(family, shape):
    """dict(blur, diameter, ref: (L [b], gx, gy, pots) in float64, err32: the float32 restatement's largest
    (loss, normalised gradient, potential) error, scaled: the scaled tolerances, tol: the tolerances the GPU
    comparison uses -- the scaled one where the float32 restatement is within a quarter of it (condition (a)),
    else (and for SINKHORN_OWN_ERROR) four times the float32 restatement's own error on this case."""
    c = case("sinkhorn", family, shape)
    b, n, m = shape[0], c.x.shape[1], c.y.shape[1]
    blur, diam = SINKHORN_BLUR * c.s, diameter(c)
    ref = [S.restated_one(c.x[i], c.y[i], blur, SINKHORN_SCALING, diam) for i in range(b)]
    err = np.zeros(3)
    for i in range(b):
        L32, gx32, gy32, p32 = S.restated_one_f32(c.x[i], c.y[i], blur, SINKHORN_SCALING, diam)
        L, gx, gy, p = ref[i]
        err = np.maximum(err, [abs(L32 - L), max(n * np.abs(gx32 - gx).max(), m * np.abs(gy32 - gy).max()),
                               np.abs(p32 - p).max()])
    scaled = sinkhorn_scaled_tolerances(diam)
    tol = tuple(t if e <= 0.25 * t and family not in SINKHORN_OWN_ERROR else 4.0 * e for t, e in zip(scaled, err))
    return dict(blur=blur, diameter=diam, ref=tuple(np.stack([np.asarray(r[k]) for r in ref]) for k in range(4)),
                err32=tuple(err), scaled=scaled, tol=tol)


def sliced_dirs(l):
    """sliced_restated.make_dirs(l) with its first two directions replaced by the z and the y axis: the z axis is
    perpendicular to `plane` and to `line` (every key of a cloud equal: the index half alone orders it), the
    y axis to `line` only."""
    dirs = SL.make_dirs(l).copy()
    dirs[0] = (0, 0, 1)
    dirs[1] = (0, 1, 0)
    return dirs


@functools.lru_cache(maxsize=None)
def sliced_reference(family, shape):
    c = case("sliced", family, shape)
    dirs = sliced_dirs(shape[3])
    return dirs, [SL.sliced_one(c.x[i], c.y[i], dirs) for i in range(shape[0])]


@functools.lru_cache(maxsize=None)
def dcd_forward(family, shape):
    """(d1, d2, i1, i2, alpha): the oracle's forward of the case and median_alpha of it -- scale-free by
    construction; where the median is 0 (identical clouds) the unit pair's alpha."""
    import oracle as O
    O.build()
    c = case("dcd", family, shape)
    d1, d2, i1, i2 = O.chamfer_forward(c.x, c.y)
    if np.median(np.concatenate([d1.ravel(), d2.ravel()])) > 0:
        alpha = D.median_alpha(d1, d2)
    else:
        alpha = dcd_forward("unit", shape)[4]
    assert np.isfinite(alpha) and alpha > 0
    return d1, d2, i1, i2, alpha


def fscore_thresholds(c):
    """FSCORE_THS times s^2, rounded to float32 (as Python floats: what the call takes)."""
    return tuple(float(F32(t * c.s * c.s)) for t in FSCORE_THS)


@functools.lru_cache(maxsize=None)
def fscore_forward(family, shape):
    """(d1, d2): the oracle's nearest squared distances of the case, read-only."""
    import oracle as O
    O.build()
    c = case("fscore", family, shape)
    d1, d2, _, _ = O.chamfer_forward(c.x, c.y)
    d1.setflags(write=False)
    d2.setflags(write=False)
    return d1, d2


@functools.lru_cache(maxsize=None)
def dcd_gradient_tolerance(family, shape, lam, tol):
    """`tol` (tests/test_dcd_gpu.py's absolute tolerance of a gradient against the oracle's chamfer_backward,
    set for unit-cube clouds) carried to the case: times the case's largest |gradient| component over the
    unit pair's, never above `tol` itself -- the gradients of scale_1e3 (2e-5) and collapsed (4e-5) are no
    larger than the plain tolerance.  One value per cloud: (tolerance for gradxyz1, for gradxyz2)."""
    import oracle as O

    def largest(f):
        c = case("dcd", f, shape)
        _, _, i1, i2, _ = dcd_forward(f, shape)
        res = dcd_reference(f, shape, lam)
        g = O.chamfer_backward(c.x, c.y, res["gd1"].astype(F32), res["gd2"].astype(F32), i1, i2)
        return [float(np.abs(v).max()) for v in g]

    return tuple(tol * min(1.0, v / u) for v, u in zip(largest(family), largest("unit")))


@functools.lru_cache(maxsize=None)
def dcd_reference(family, shape, lam):
    d1, d2, i1, i2, alpha = dcd_forward(family, shape)
    return D.evaluate(d1, d2, i1, i2, alpha, lam, False)
