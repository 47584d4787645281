"""The contract of pcm_sinkhorn_loss (include/pcm.h) restated in numpy: the
debiased Sinkhorn divergence (p = 2, uniform weights) of two clouds by the
symmetric averaged Sinkhorn loop with epsilon-scaling and a last extrapolation
step, its gradients by the envelope rule, and the potentials.  `restated_one`
is float64 from the float32 inputs; `restated_one_f32` follows the kernel's
steps in float32 (base 2, the same three constants a step, a running maximum)
with numpy's exp2 / log2 in place of the hardware's.  geomloss is not installed
here: the algorithm is the published one and is NOT verified against geomloss.
Also here: the shapes, settings and clouds the tests share, the modelled
defects, and the two tolerances of the GPU comparison."""
import functools
import math

import numpy as np

# csrc/sinkhorn.hip (the CPU test checks them against the source)
ROWS, TILE, WAVES = 128, 1024, 8
MAX_POINTS, MAX_STEPS = 16384, 128

# (blur, scaling): schedules of T = 8 and T = 10 entries at D = sqrt(3)
SETTINGS = [(0.05, 0.5), (0.1, 0.7)]
DIAMETER = float(np.float32(math.sqrt(3.0)))  # the unit cube's diagonal, as the float the library is given

# (b, n, m) around the edges of ROWS rows and TILE columns
SHAPES = [(1, 1, 1), (2, 65, 63), (2, 129, 1), (2, 127, 128),
          (2, 300, 1025), (1, 1024, 1024), (1, 1023, 130), (1, 2049, 5)]

# Tolerances of the float32 kernel against the float64 restatement: TOL_LOSS absolute on loss_out, TOL_GRAD
# on n |grad1 - ref| and m |grad2 - ref| (the gradient of a point carries its weight 1/n or 1/m), TOL_POT
# absolute on the potentials.  They are NOT taken from what any kernel gives: tests/test_sinkhorn_cpu.py
# holds them between two conditions -- (a) the float32 restatement below stays within a quarter of each on
# every shape and setting, (b) each modelled defect moves the float64 result by more than ten times the
# tolerance on every shape with n + m >= 128.
TOL_LOSS = 1e-6
TOL_GRAD = 1e-4
TOL_POT = 1e-5


def schedule(blur, scaling, diameter):
    """The epsilon list of pcm_sinkhorn_schedule, in double from the float32 arguments."""
    blur, scaling, diameter = (float(np.float32(v)) for v in (blur, scaling, diameter))
    lo, hi, step = 2.0 * math.log(blur), 2.0 * math.log(diameter), 2.0 * math.log(scaling)
    eps = [diameter * diameter]
    k = 1
    while hi + (k - 1) * step > lo:
        eps.append(math.exp(hi + (k - 1) * step))
        k += 1
    eps.append(blur * blur)
    return eps


@functools.lru_cache(maxsize=None)
def make_clouds(b, n, m, seed=0):
    """Two float32 clouds in the unit cube: x uniform over it, y uniform over a
    cube of edge 0.25 in one corner (the clouds of tests/kernel_loss_restated.py)."""
    rng = np.random.default_rng(1000 * n + m + seed)
    x = rng.random((b, n, 3), dtype=np.float32)
    y = (rng.random((b, m, 3), dtype=np.float32) * np.float32(0.25) + np.float32(0.75)).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _cost(p, q):
    return 0.5 * sum((p[:, None, c] - q[None, :, c]) ** 2 for c in range(3))


def _lse(z):
    """log sum_j exp(z_ij) relative to the row maximum; an empty row gives -inf."""
    if z.shape[1] == 0:
        return np.full(z.shape[0], -np.inf)
    mx = z.max(axis=1)
    return mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))


def softmin(eps, C, h):
    return -eps * _lse(h[None, :] - C / eps)


def _softmax(z):
    w = np.exp(z - z.max(axis=1)[:, None])
    return w / w.sum(axis=1)[:, None]


def sinkhorn_one(x, y, eps_list, skip_cols=None):
    """The loop of the contract in float64 on two clouds [n, 3], [m, 3] for the
    schedule eps_list.  Returns x, y (float64), the four extrapolated
    potentials (F_ba, F_aa, G_ab, G_bb) and the softmax weights (P, Q) of x's
    rows and (Pt, Qt) of y's.  skip_cols = (cloud, start, stop): the CROSS
    softmins leave those columns of cloud 0 (x) or 1 (y) out, in every step --
    what a kernel that dropped a tile of the other cloud would compute."""
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    n, m = len(x), len(y)
    la, lb = np.full(n, -math.log(n)), np.full(m, -math.log(m))
    kx, ky = np.ones(n, bool), np.ones(m, bool)
    if skip_cols is not None:
        (kx, ky)[skip_cols[0]][skip_cols[1]:skip_cols[2]] = False
    Cxy, Cxx, Cyy = _cost(x, y), _cost(x, x), _cost(y, y)
    Cxy_c, Cyx_c = Cxy[:, ky], Cxy.T[:, kx]  # the cross softmins' columns

    def four(eps, f_ba, g_ab, f_aa, g_bb):
        return (softmin(eps, Cxy_c, (lb + g_ab / eps)[ky]), softmin(eps, Cyx_c, (la + f_ba / eps)[kx]),
                softmin(eps, Cxx, la + f_aa / eps), softmin(eps, Cyy, lb + g_bb / eps))

    with np.errstate(all="ignore"):  # a cloud with every column left out gives infinities, on purpose
        e0 = eps_list[0]
        f_ba, g_ab, f_aa, g_bb = four(e0, np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m))
        for eps in eps_list:
            ft_ba, gt_ab, ft_aa, gt_bb = four(eps, f_ba, g_ab, f_aa, g_bb)
            f_ba, g_ab = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab)
            f_aa, g_bb = 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
        eps = eps_list[-1]
        F_ba, G_ab, F_aa, G_bb = four(eps, f_ba, g_ab, f_aa, g_bb)
        weights = None
        if skip_cols is None:
            weights = (_softmax((lb + g_ab / eps)[None, :] - Cxy / eps), _softmax((la + f_aa / eps)[None, :] - Cxx / eps),
                       _softmax((la + f_ba / eps)[None, :] - Cxy.T / eps), _softmax((lb + g_bb / eps)[None, :] - Cyy / eps))
    return {"x": x, "y": y, "F_ba": F_ba, "F_aa": F_aa, "G_ab": G_ab, "G_bb": G_bb, "weights": weights,
            "averaged": (f_ba, g_ab, f_aa, g_bb)}


def loss_from(res, skip_rows=None):
    """sum_i a (F_ba - F_aa)_i + sum_j b (G_ab - G_bb)_j; skip_rows = (cloud, start, stop) leaves those rows out."""
    n, m = len(res["x"]), len(res["y"])
    rows = [np.ones(n, bool), np.ones(m, bool)]
    if skip_rows is not None:
        rows[skip_rows[0]][skip_rows[1]:skip_rows[2]] = False
    with np.errstate(all="ignore"):
        tx = (res["F_ba"] - res["F_aa"]) / n
        ty = (res["G_ab"] - res["G_bb"]) / m
        return float(tx[rows[0]].sum() + ty[rows[1]].sum())


def grads_from(res):
    """grad_x[i] = a (sum_k Q_ik x_k - sum_j P_ij y_j), grad_y with the roles swapped."""
    x, y = res["x"], res["y"]
    P, Q, Pt, Qt = res["weights"]
    return (Q @ x - P @ y) / len(x), (Qt @ y - Pt @ x) / len(y)


def potentials_from(res):
    """[n + m, 2]: (F_cross, F_own) of every row of x || y, as potentials_out has them."""
    return np.concatenate([np.stack([res["F_ba"], res["F_aa"]], 1), np.stack([res["G_ab"], res["G_bb"]], 1)])


def restated_one(x, y, blur, scaling, diameter=DIAMETER, eps_list=None):
    """(L, grad_x, grad_y, potentials [n + m, 2]) of one pair of clouds in float64."""
    res = sinkhorn_one(x, y, schedule(blur, scaling, diameter) if eps_list is None else eps_list)
    gx, gy = grads_from(res)
    return loss_from(res), gx, gy, potentials_from(res)


@functools.lru_cache(maxsize=None)
def restated(b, n, m, blur, scaling, seed=0):
    """(L [b], grad_x [b, n, 3], grad_y [b, m, 3], potentials [b, n + m, 2]) of make_clouds(b, n, m, seed)."""
    x, y = make_clouds(b, n, m, seed)
    res = [restated_one(x[i], y[i], blur, scaling) for i in range(b)]
    return tuple(np.stack([np.asarray(r[k]) for r in res]) for k in range(4))


# ---------------------------------------------------------------------------
# The kernel's steps in float32
# ---------------------------------------------------------------------------
F32 = np.float32
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def _d2_f32(p, q):
    """The pinned order fmaf(dz, dz, fmaf(dy, dy, dx dx)), each fused step formed in double and rounded once."""
    d = [(p[:, None, c] - q[None, :, c]).astype(F32) for c in range(3)]
    s = (d[0] * d[0]).astype(F32)
    s = (d[1].astype(np.float64) * d[1] + s).astype(F32)
    return (d[2].astype(np.float64) * d[2] + s).astype(F32), d


def _softmin_f32(d2, diffs, pot, lw, eps, want_weights=False):
    """(max + log2 sum 2^(t - max)) * fl(-eps ln 2) with t = fmaf(d2, c, h2), h2 = fmaf(pot, s, lw)."""
    c, s, out = F32(-LOG2E / (2.0 * eps)), F32(LOG2E / eps), F32(-eps * LN2)
    h2 = (pot.astype(np.float64) * float(s) + float(lw)).astype(F32) if pot is not None else np.full(d2.shape[1], lw, F32)
    t = (d2.astype(np.float64) * float(c) + h2[None, :].astype(np.float64)).astype(F32)
    mx = t.max(axis=1)
    w = np.exp2((t - mx[:, None]).astype(F32)).astype(F32)
    S = w.sum(axis=1, dtype=F32)
    F = ((mx + np.log2(S).astype(F32)).astype(F32) * out).astype(F32)
    if not want_weights:
        return F
    V = np.stack([(w * diffs[k]).sum(axis=1, dtype=F32) / S for k in range(3)], 1).astype(F32)  # sum P (p - q)
    return F, V


def restated_one_f32(x, y, blur, scaling, diameter=DIAMETER):
    """(L, grad_x, grad_y, potentials) as restated_one, every step of the scans in float32."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    n, m = len(x), len(y)
    eps_list = schedule(blur, scaling, diameter)
    lw1, lw2 = F32(-math.log2(n)), F32(-math.log2(m))
    (dxy, fxy), (dyx, fyx), (dxx, fxx), (dyy, fyy) = _d2_f32(x, y), _d2_f32(y, x), _d2_f32(x, x), _d2_f32(y, y)

    def four(eps, f_ba, g_ab, f_aa, g_bb, last=False):
        return (_softmin_f32(dxy, fxy, g_ab, lw2, eps, last), _softmin_f32(dyx, fyx, f_ba, lw1, eps, last),
                _softmin_f32(dxx, fxx, f_aa, lw1, eps, last), _softmin_f32(dyy, fyy, g_bb, lw2, eps, last))

    f_ba, g_ab, f_aa, g_bb = four(eps_list[0], None, None, None, None)
    for eps in eps_list:
        ft_ba, gt_ab, ft_aa, gt_bb = four(eps, f_ba, g_ab, f_aa, g_bb)
        f_ba, g_ab = F32(0.5) * (f_ba + ft_ba), F32(0.5) * (g_ab + gt_ab)
        f_aa, g_bb = F32(0.5) * (f_aa + ft_aa), F32(0.5) * (g_bb + gt_bb)
    (F_ba, Vxy), (G_ab, Vyx), (F_aa, Vxx), (G_bb, Vyy) = four(eps_list[-1], f_ba, g_ab, f_aa, g_bb, True)
    L = float(np.float32((F_ba.astype(np.float64) - F_aa).sum() / n + (G_ab.astype(np.float64) - G_bb).sum() / m))
    gx = (F32(1.0 / n) * (Vxy - Vxx)).astype(F32)
    gy = (F32(1.0 / m) * (Vyx - Vyy)).astype(F32)
    pots = np.concatenate([np.stack([F_ba, F_aa], 1), np.stack([G_ab, G_bb], 1)])
    return L, gx, gy, pots
