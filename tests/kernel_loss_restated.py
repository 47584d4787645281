"""The contract of pcm_kernel_loss (include/pcm.h) restated in numpy float64:
the kernel norm 1/2 |alpha - beta|^2_k of two uniformly weighted clouds and its
gradient in both, for the Gaussian, Laplacian and energy kernels, computed from
the float32 inputs.  A coincident pair (r = 0) adds nothing to a Laplacian or
energy gradient.  Also here: the shapes and clouds the tests share, and the
error bounds of the float32 kernel against this restatement -- derived below
from the roundings the contract names, not tuned to what any kernel gives."""
import functools

import numpy as np

GAUSSIAN, LAPLACIAN, ENERGY = 0, 1, 2
KERNELS = (GAUSSIAN, LAPLACIAN, ENERGY)
KERNEL_NAMES = {GAUSSIAN: "gaussian", LAPLACIAN: "laplacian", ENERGY: "energy"}
BLURS = (0.2, 1.0)

# csrc/kernel_loss.hip (the CPU test checks them against pcm_hip's constants)
ROWS, TILE, WAVES = 128, 1024, 8

# (b, n, m): the batched shapes, then b = 1 one below, at and one above ROWS (for n, and for n + m) and
# TILE (for m, and for n)
SHAPES = [(2, 1, 1), (2, 3, 2), (2, 64, 64), (2, 65, 63), (2, 257, 255), (2, 300, 1025),
          (1, ROWS - 1, 40), (1, ROWS, 40), (1, ROWS + 1, 40),
          (1, ROWS // 2, ROWS // 2 - 1), (1, ROWS // 2, ROWS // 2), (1, ROWS // 2, ROWS // 2 + 1),
          (1, 5, TILE - 1), (1, 5, TILE), (1, 5, TILE + 1),
          (1, TILE - 1, 5), (1, TILE, 5), (1, TILE + 1, 5)]
assert len(SHAPES) <= 40


@functools.lru_cache(maxsize=None)
def make_clouds(b, n, m, seed=0):
    """Two float32 clouds in the unit cube: x uniform over it, y uniform over a
    cube of edge 0.25 in one corner -- two different distributions, so that the
    loss is far above its rounding error and every block of rows and tile of
    columns carries a visible share of it (the CPU test checks that)."""
    rng = np.random.default_rng(1000 * n + m + seed)
    x = rng.random((b, n, 3), dtype=np.float32)
    y = (rng.random((b, m, 3), dtype=np.float32) * np.float32(0.25) + np.float32(0.75)).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _pairs(p, q, kernel, sigma):
    """k [P, Q] and the derivative's g [P, Q]: grad_p k(p, q) = C g (p - q)."""
    d2 = sum((p[:, None, c] - q[None, :, c]) ** 2 for c in range(3))
    r = np.sqrt(d2)
    inv = np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0), 0.0)  # the r = 0 rule
    if kernel == GAUSSIAN:
        k = np.exp(-d2 / (2.0 * sigma * sigma))
        return k, k
    if kernel == LAPLACIAN:
        k = np.exp(-r / sigma)
        return k, k * inv
    return -r, inv


def derivative_factor(kernel, sigma):
    return {GAUSSIAN: -1.0 / (sigma * sigma), LAPLACIAN: -1.0 / sigma, ENERGY: -1.0}[kernel]


def pair_matrices(x, y, kernel, blur):
    """The float64 clouds and the (k, g) matrices of the pairs x-x, y-y and x-y of two clouds [n, 3], [m, 3]."""
    sigma = float(np.float32(blur))
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    return x, y, _pairs(x, x, kernel, sigma), _pairs(y, y, kernel, sigma), _pairs(x, y, kernel, sigma)


def loss_from(mats, skip_cols=None, skip_rows=None):
    """L in float64 from pair_matrices' result.  skip_cols = (cloud, start,
    stop): every row sum leaves out those columns of cloud 0 (x) or 1 (y);
    skip_rows likewise leaves those rows' terms out of L: what a kernel that
    dropped a tile or a block would compute."""
    x, y, (kxx, _), (kyy, _), (kxy, _) = mats
    n, m = len(x), len(y)
    a, b = 1.0 / n, 1.0 / m
    keep = [np.ones(n, bool), np.ones(m, bool)]
    if skip_cols is not None:
        keep[skip_cols[0]][skip_cols[1]:skip_cols[2]] = False
    rows = [np.ones(n, bool), np.ones(m, bool)]
    if skip_rows is not None:
        rows[skip_rows[0]][skip_rows[1]:skip_rows[2]] = False
    # row p of the cloud of weight w: 1/2 w (w S_own - w_o S_other)
    tx = 0.5 * a * (a * kxx[:, keep[0]].sum(1) - b * kxy[:, keep[1]].sum(1))
    ty = 0.5 * b * (b * kyy[:, keep[1]].sum(1) - a * kxy[keep[0], :].sum(0))
    return float(tx[rows[0]].sum() + ty[rows[1]].sum())


def restated_one(x, y, kernel, blur):
    """(L, grad_x, grad_y) of one pair of clouds [n, 3], [m, 3] in float64."""
    mats = pair_matrices(x, y, kernel, blur)
    x, y, (_, gxx), (_, gyy), (_, gxy) = mats
    a, b = 1.0 / len(x), 1.0 / len(y)
    C = derivative_factor(kernel, float(np.float32(blur)))

    def v(p, g, q):  # sum_q g (p - q)
        return p * g.sum(1)[:, None] - g @ q

    gx = C * a * (a * v(x, gxx, x) - b * v(x, gxy, y))
    gy = C * b * (b * v(y, gyy, y) - a * v(y, gxy.T, x))
    return loss_from(mats), gx, gy


def grads_from(mats, kernel, blur, keep=None):
    """(grad_x, grad_y) in float64 from pair_matrices' result, restated_one's formula.  keep = (mask over x's
    points, mask over y's): every point's sums run over those columns only -- what a kernel that dropped a
    tile of columns would compute (loss_from's skip_cols, for the gradients)."""
    x, y, (_, gxx), (_, gyy), (_, gxy) = mats
    a, b = 1.0 / len(x), 1.0 / len(y)
    C = derivative_factor(kernel, float(np.float32(blur)))
    kx, ky = (np.ones(len(x), bool), np.ones(len(y), bool)) if keep is None else keep

    def v(p, g, q):  # sum_q g (p - q)
        return p * g.sum(1)[:, None] - g @ q

    gx = C * a * (a * v(x, gxx[:, kx], x[kx]) - b * v(x, gxy[:, ky], y[ky]))
    gy = C * b * (b * v(y, gyy[:, ky], y[ky]) - a * v(y, gxy.T[:, kx], x[kx]))
    return gx, gy


@functools.lru_cache(maxsize=None)
def restated(b, n, m, kernel, blur, seed=0):
    """(L [b], grad_x [b, n, 3], grad_y [b, m, 3]) of make_clouds(b, n, m, seed), computed once."""
    x, y = make_clouds(b, n, m, seed)
    res = [restated_one(x[i], y[i], kernel, blur) for i in range(b)]
    return (np.array([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]))


# ---------------------------------------------------------------------------
# Error bounds of the float32 kernel against the float64 restatement
# ---------------------------------------------------------------------------
# u = 2^-24, the unit roundoff of float32.  Every bound is first order in u; SLACK covers the second-order
# terms (the longest chain is 2055 additions: 2055 u = 1.2e-4) and the double sums (1e-16 a step).
U = 2.0 ** -24
# the one constant IEEE does not give: the relative error allowed to the hardware exp2
EPS_EXP = 2.0 ** -21
SLACK = 1.001
# d2 = fmaf(dz,dz,fmaf(dy,dy,dx*dx)): a difference is within u, its square within 2 u, dx*dx rounded 3 u;
# each fmaf adds a non-negative square (2 u) and rounds once, so the sum's relative error is the larger
# of its parts' plus u: 4 u, then 5 u.
RHO_D2 = 5.0
# r = sqrtf(d2), correctly rounded: half of d2's error and its own rounding
RHO_R = RHO_D2 / 2 + 1
# the exponent t: d2 (or r) times the constant c, c rounded once (u) and the product once (u)
RHO_T = {GAUSSIAN: RHO_D2 + 2, LAPLACIAN: RHO_R + 2}
# k = 2^t: an error rho u |t| in t moves k by k ln2 |t| rho u, and k ln2 |t| = s e^-s <= 1/e = 0.37 for
# s = -t ln2 >= 0; the exp2 itself adds EPS_EXP k and k <= 1: a term of a row sum S is within
K_ERR = {GAUSSIAN: 0.37 * RHO_T[GAUSSIAN] + EPS_EXP / U, LAPLACIAN: 0.37 * RHO_T[LAPLACIAN] + EPS_EXP / U}  # units of u


def chain(n, m):
    """The longest chain of float32 additions behind a row sum (include/pcm.h)."""
    share = TILE // WAVES  # wave 0's columns of every tile, then the additions that merge the waves
    return max(share * (c // TILE) + min(share, c % TILE) + WAVES - 1 for c in (n, m))


def diameter(x, y):
    """An upper bound of every pair distance of the two clouds: the bounding box's diagonal."""
    pts = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3), np.asarray(y, np.float64).reshape(-1, 3)])
    return float(np.linalg.norm(pts.max(0) - pts.min(0)))


def loss_bound(kernel, n, m, diam=None):
    """|L - L64| <=.  The pair weights 1/2 a a, 1/2 b b (n^2, m^2 pairs) and a b (n m pairs, each seen from
    both clouds at half weight) sum to 2.  A term is within K_ERR u (k <= 1), a row sum of terms in [0, 1]
    within chain u times their number: 2 (K_ERR + chain) u; the double sum is rounded once to float32 and
    |L| <= 1: one more u.  Energy: a term -r is within RHO_R u r, r <= diam and |L| <= diam:
    (2 (RHO_R + chain) + 1) u diam."""
    ch = chain(n, m)
    if kernel == ENERGY:
        return SLACK * (2 * (RHO_R + ch) + 1) * U * diam
    return SLACK * (2 * (K_ERR[kernel] + ch) + 1) * U


def grad_bound(kernel, n, m, blur):
    """(bound of a component of grad_x, of grad_y).  Row p of the cloud of weight w collects
    C w (w V_own - w_o V_other), V = sum g (p - q)_c by one fmaf a term; the weights w sum_q w' over both
    clouds come to 2 w.
    Gaussian, per term k dx with |dx| <= r, s = d2 / (2 sigma^2): |dx| k <= sigma sqrt(2 s) e^-s <= 0.61
    sigma; k's error from its exponent, r k s rho_t u = sigma sqrt(2) s^1.5 e^-s rho_t u <= 0.58 sigma rho_t
    u; the exp2's and dx's own add (EPS_EXP + u) 0.61 sigma.  The chain adds chain u 0.61 sigma a term.
    The two coefficients are rounded once each, their products and the last fmaf once: 3 u of
    |C| w 2 * 0.61 sigma.  With |C| = 1 / sigma^2:
        2 (w / sigma) u (0.58 rho_t + 0.61 (EPS_EXP / u + 1 + chain + 3)).
    Laplacian, per term k (dx / r), at most 1: k is within K_ERR u, dx / r within (1 + RHO_R + 1) u, and
    |C| = 1 / sigma: 2 (w / sigma) u (K_ERR + RHO_R + 2 + chain + 3).
    Energy, per term dx / r, C = -1: 2 w u (RHO_R + 2 + chain + 3).
    (A difference whose square underflows float32 is outside these bounds; the tests' clouds have none.)"""
    sigma = float(np.float32(blur))
    ch = chain(n, m)
    if kernel == GAUSSIAN:
        per = (0.58 * RHO_T[GAUSSIAN] + 0.61 * (EPS_EXP / U + 1 + ch + 3)) / sigma
    elif kernel == LAPLACIAN:
        per = (K_ERR[LAPLACIAN] + RHO_R + 2 + ch + 3) / sigma
    else:
        per = RHO_R + 2 + ch + 3
    return SLACK * 2 * per * U / n, SLACK * 2 * per * U / m
