"""numpy restatement of pcm_dcd_loss's contract (include/pcm.h): distances and
lowest-index argmins from the oracle's chamfer_forward (the project's pinned
checker), hit counts by np.bincount, and the terms, the loss, cd_p, cd_t, the
graddists and the analytic gradient in float64.  Test infrastructure only: the
GPU tests compare the kernel with it, the CPU tests check it against a
brute-force double loop, central differences and identities.

Inputs.  Uniform random float32 clouds in the unit cube; alpha is set per case
to 1 / median of all nearest-neighbour squared distances of the case, rounded
to float32, so that exp(-alpha d) is spread over (0, 1) and the counts matter:
``restated`` asserts, for every case but the 1-point ones, that the mean of
exp(-alpha d) lies in [0.2, 0.6] and that at least half of the queries hit a
target whose count is not 1.  A saturated or density-blind case cannot pass for
a test.

Error bounds (what a float32 output may differ from this float64 value by).
They follow the pinned chain of the header, u = 2^-24 a rounding:
    a = fl(alpha d)          a (1 + u).  Through the exponential this is a
                             RELATIVE error a u of e (exp(-a (1 + u)) =
                             exp(-a) exp(-a u)): the term proportional to
                             alpha d.
    e = expf(-a)             the device library's expf; the OpenCL full profile
                             it is built to allows 3 ulp = 6 u (HIP documents 1).
    p                        exact for lambda in {0, 1} (a count up to 16384 is
                             a float32); else powf, 16 ulp = 32 u by the same
                             profile (HIP documents 1).
    p + 1e-6f, 1 / (.), * r, r itself (one float32 division; this file keeps
                             r = Q / T exact), e * w: five roundings, 5 u.
  so  |err g| <= RHO g,  RHO = (a + K) u (1 + 2^-10),  K = 11, or 43 with powf;
  the factor (1 + 2^-10) covers the second-order terms ((a + K) u < 2^-10 for
  a < 16000, beyond which exp(-a) is 0 in float32 and in float64 alike).
  Beyond a = 16000 (one outlier far from a cloud whose alpha comes from the
  median: tests/geometry_cases.py's far_point has a = 1e6) RHO itself is no
  longer small, but it multiplies nothing: the float32 a = fl(alpha d) is at
  least 16000 (1 - u) > 745, so expf(-a) and the double exp alike return 0
  exactly, g = 0, term = fl(1 - 0) = 1 and graddist = 0 in both precisions,
  and the bounds below reduce to their g-free parts (2^-126 and u |term|, and
  alpha 2^-126 / (2 Q) + 2^-149), which such a term meets with error 0.  All
  that is needed of a is that it be finite, i.e. alpha d below 3.4e38.
  tests/test_geometry_cpu.py asserts e = g = graddist = 0 and term = 1 there
  for the float32 and the float64 evaluation.
  A g below the normal range may lose its last bits or be flushed: + 2^-126.
    term = fl(1 - g)         |err term| <= RHO g + 2^-126 + u |1 - g|.
    loss                     the mean of the terms' errors of each direction,
                             halved (the sums are in double: 2^-50 of the sum of
                             |term| stands for them), and one rounding u |loss|.
    graddist = fl(fl(alpha g) / (2 Q))
                             |err| <= (RHO + 2 u (1 + 2^-10)) graddist
                                      + alpha 2^-126 / (2 Q) + 2^-149.
    cd_p                     sqrtf is correctly rounded: u sqrt(d) a term, and
                             one rounding: 2 u cd_p (1 + 2^-20).
    cd_t                     the float32 distances are added exactly in double
                             (to 2^-53 n): one rounding, u cd_t (1 + 2^-20).
None of this is tuned to a device's output; test_dcd_cpu.py checks that a
float32 evaluation in numpy stays inside, and that each modelled defect leaves
by more than ten bounds.
"""
import numpy as np

U32 = 2.0 ** -24
EPS = float(np.float32(1e-6))
TINY = 2.0 ** -126
MAX_POINTS = 16384

# (b, n, m) of the GPU comparison; (16, 4096, 4096) is the smallest that takes the grid forward
SHAPES = [(2, 1, 1), (3, 7, 5), (2, 48, 80), (2, 100, 33), (2, 1000, 333), (2, 1024, 1024), (2, 1025, 1023),
          (2, 128, 1024), (16, 4096, 4096), (1, 16384, 16384)]
LAMBDAS = [1.0, 0.5, 0.0]


def cases():
    """(b, n, m, lambda, non_reg): every shape with every lambda, non_reg on and off where n != m."""
    return [(b, n, m, lam, nr) for b, n, m in SHAPES for lam in LAMBDAS for nr in ((False, True) if n != m else (False,))]


def make_clouds(b, n, m, seed=0):
    """Two clouds uniform in the unit cube: float32."""
    rng = np.random.default_rng(2000 * seed + 11 * n + 5 * m + b)
    return rng.random((b, n, 3), dtype=np.float32), rng.random((b, m, 3), dtype=np.float32)


def median_alpha(d1, d2):
    """float32 1 / median of all nearest-neighbour squared distances."""
    return np.float32(1.0 / np.median(np.concatenate([d1.ravel(), d2.ravel()]).astype(np.float64)))


def counts(idx, targets, drop_tail=False):
    """[b, targets] int64 hit counts of an argmin array [b, q].  drop_tail
    (a modelled defect): the last q mod 64 queries left out."""
    use = idx.shape[1] - (idx.shape[1] % 64 if drop_tail else 0)
    return np.stack([np.bincount(row[:use], minlength=targets) for row in idx]).astype(np.int64)


def ratio(q, t, non_reg):
    return max(1.0, q / t) if non_reg else q / t


def evaluate(d1, d2, i1, i2, alpha, lam, non_reg, dtype=np.float64, defect=None):
    """The contract over given distances and argmins, in ``dtype`` (float32: every
    step rounded, as the pinned chain): dict(loss [b], cd [b, 2], gd1, gd2,
    c1, c2, term1, term2, g1, g2, a1, a2).  ``defect`` models one of: "swap_r",
    "cross_counts", "drop_tail", "ignore_lambda", "ignore_non_reg"."""
    b, n = d1.shape
    m = d2.shape[1]
    c1 = counts(i2, n, defect == "drop_tail")  # hits on cloud 1's points
    c2 = counts(i1, m, defect == "drop_tail")
    if defect == "ignore_lambda":
        lam = 1.0
    if defect == "ignore_non_reg":
        non_reg = False
    r1, r2 = ratio(n, m, non_reg), ratio(m, n, non_reg)
    if defect == "swap_r":
        r1, r2 = r2, r1
    alpha, lam = dtype(np.float32(alpha)), dtype(np.float32(lam))
    out = dict(c1=c1, c2=c2)
    rows = np.arange(b)[:, None]
    for tag, d, idx, hist, other, r, q in (("1", d1, i1, c2, c1, r1, n), ("2", d2, i2, c1, c2, r2, m)):
        if defect == "cross_counts":  # the other direction's histogram, read at this direction's argmins
            c = other[rows, np.minimum(idx, other.shape[1] - 1)].astype(dtype)
        else:
            c = hist[rows, idx].astype(dtype)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            a = alpha * d.astype(dtype)
            e = np.exp(-a)
            p = c if lam == 1 else (np.ones_like(c) if lam == 0 else np.power(c, lam))
            w = (dtype(1) / (p + dtype(EPS))) * dtype(r)
            g = e * w
            out["a" + tag], out["g" + tag], out["term" + tag] = a, g, dtype(1) - g
            out["gd" + tag] = (alpha * g) / dtype(2 * q)
    d1, d2 = d1.astype(np.float64), d2.astype(np.float64)
    with np.errstate(invalid="ignore"):
        out["loss"] = (out["term1"].mean(axis=1, dtype=np.float64) + out["term2"].mean(axis=1, dtype=np.float64)) / 2
        out["cd"] = np.stack([(np.sqrt(d1).mean(axis=1) + np.sqrt(d2).mean(axis=1)) / 2,
                              d1.mean(axis=1) + d2.mean(axis=1)], axis=1)
    return out


def bounds(res, alpha, lam, n, m):
    """(loss [b], cd [b, 2], gd1 [b, n], gd2 [b, m]) bounds of a float64 result (see the module text)."""
    K = 11.0 if float(lam) in (0.0, 1.0) else 43.0
    alpha = float(np.float32(alpha))
    second = 1.0 + 2.0 ** -10
    loss = np.zeros(len(res["loss"]))
    gds = []
    for tag, q in (("1", n), ("2", m)):
        a, g, term, gd = (np.asarray(res[k + tag], np.float64) for k in ("a", "g", "term", "gd"))
        rho = (a + K) * U32 * second
        err_term = rho * g + TINY + U32 * np.abs(term)
        loss += 0.5 * (err_term.mean(axis=1) + 2.0 ** -50 * np.abs(term).mean(axis=1))
        gds.append((rho + 2 * U32 * second) * gd + alpha * TINY / (2 * q) + 2.0 ** -149)
    loss += U32 * np.abs(res["loss"])
    cd = np.abs(res["cd"]) * np.array([2 * U32, U32]) * (1 + 2.0 ** -20)
    return loss, cd, gds[0], gds[1]


def gradients(x, y, i1, i2, gd1, gd2):
    """float64 pcm_chamfer_backward of the graddists: (gradxyz1 [b, n, 3], gradxyz2 [b, m, 3])."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for bi in range(len(x)):
        t1 = 2.0 * gd1[bi][:, None] * (x[bi] - y[bi][i1[bi]])  # direction 1: query j, target i1[j]
        t2 = 2.0 * gd2[bi][:, None] * (y[bi] - x[bi][i2[bi]])
        gx[bi] += t1
        np.add.at(gy[bi], i1[bi], -t1)
        gy[bi] += t2
        np.add.at(gx[bi], i2[bi], -t2)
    return gx, gy


def brute_forward(x, y):
    """float64 squared distances and lowest-index argmins by a double loop: one element."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d1, i1 = np.empty(len(x)), np.empty(len(x), np.int32)
    d2, i2 = np.empty(len(y)), np.empty(len(y), np.int32)
    for d, i, p, q in ((d1, i1, x, y), (d2, i2, y, x)):
        for j in range(len(p)):
            best, at = np.inf, 0
            for k in range(len(q)):
                v = float(((q[k] - p[j]) ** 2).sum())
                if v < best:
                    best, at = v, k
            d[j], i[j] = best, at
    return d1, d2, i1, i2


def brute_loss(x, y, alpha, lam, non_reg):
    """The contract's loss of one element straight from its text, float64, plain Python sums."""
    d1, d2, i1, i2 = brute_forward(x, y)
    n, m = len(x), len(y)
    total = 0.0
    for d, idx, q, t in ((d1, i1, n, m), (d2, i2, m, n)):
        r = ratio(q, t, non_reg)
        acc = 0.0
        for j in range(q):
            c = sum(1 for v in idx if v == idx[j])
            acc += 1.0 - np.exp(-float(alpha) * d[j]) * r / (float(c) ** float(lam) + EPS)
        total += acc / q
    return total / 2, (d1, d2, i1, i2)


_cache = {}


def forward(b, n, m, seed=0):
    """(x, y, d1, d2, i1, i2, alpha) of a case: the oracle's forward, computed once and shared (read-only)."""
    key = (b, n, m, seed)
    if key not in _cache:
        import oracle as O
        O.build()
        x, y = make_clouds(b, n, m, seed)
        d1, d2, i1, i2 = O.chamfer_forward(x, y)
        alpha = median_alpha(d1, d2)
        if n > 1 and m > 1:
            with np.errstate(under="ignore"):
                e = np.exp(-float(alpha) * np.concatenate([d1.ravel(), d2.ravel()]).astype(np.float64))
            c1, c2 = counts(i2, n), counts(i1, m)
            rows = np.arange(b)[:, None]
            hit = np.concatenate([c2[rows, i1].ravel(), c1[rows, i2].ravel()])
            assert 0.2 <= e.mean() <= 0.6, (key, e.mean())
            assert (hit != 1).mean() >= 0.5, (key, (hit != 1).mean())
        _cache[key] = (x, y, d1, d2, i1, i2, alpha)
    return _cache[key]


_results = {}


def restated(b, n, m, lam, non_reg, seed=0):
    """forward(...) + (the float64 result dict,) shared among the tests (read-only)."""
    key = (b, n, m, float(lam), bool(non_reg), seed)
    if key not in _results:
        x, y, d1, d2, i1, i2, alpha = forward(b, n, m, seed)
        _results[key] = evaluate(d1, d2, i1, i2, alpha, lam, non_reg)
    return forward(b, n, m, seed) + (_results[key],)
