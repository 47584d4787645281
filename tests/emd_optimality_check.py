"""The auction's guarantee for one cloud pair, checked without the oracle.

Shared by tests/test_emd_optimality.py (unit-cube clouds, fixed slack) and the
stress family (tests/test_emd_stress_cpu.py, tests/test_emd_stress_gpu.py),
whose slack scales with the magnitude of the case's values.
"""
from collections import namedtuple

import numpy as np
from scipy.optimize import linear_sum_assignment

EpsOptimal = namedtuple("EpsOptimal", "excess worst_gap magnitude slack")


def distances(x1, x2):
    """float64 ||x1_j - x2_k|| of the float32 inputs, [n, n], in row blocks."""
    n = x1.shape[0]
    p, q = x1.astype(np.float64), x2.astype(np.float64)
    dist = np.empty((n, n))
    for lo in range(0, n, 512):
        dif = p[lo:lo + 512, None, :] - q[None, :, :]
        dist[lo:lo + 512] = np.sqrt((dif * dif).sum(-1))
    return dist


def check_eps_optimal(x1, x2, ass, price, eps, slack=None, solve=True):
    """One batch element: bijection, eps-CS at the final prices (each point's
    object is within eps + slack of its best value 3 - ||x_j - y_k|| - price_k)
    and, if `solve`, OPT <= cost <= OPT + n * (eps + slack) against
    scipy.optimize.linear_sum_assignment on the same float64 distances.

    slack=None is 4 float32 ulps of M = 3 + max distance + max price.  Values,
    prices and increments are float32 of magnitude at most M: a winning bid's
    price += best - better + eps carries at most about 2 ulp(M) of rounding,
    the float64 recomputation of the two values compared at most 1 more; the
    fourth is spare.

    Returns (excess = (cost - OPT) / (n * eps) or None, worst gap, M, slack)."""
    n = x1.shape[0]
    np.testing.assert_array_equal(np.sort(ass), np.arange(n))  # converged: a bijection
    dist = distances(x1, x2)
    big = 3.0 + float(dist.max()) + float(np.abs(price).max())
    if slack is None:
        slack = 4 * 2.0 ** -24 * big
    val = (3.0 - dist) - price.astype(np.float64)[None, :]
    rows = np.arange(n)
    gap = val.max(1) - val[rows, ass]
    assert gap.max() <= eps + slack, f"eps-CS broken: worst gap {gap.max()} > eps {eps} + slack {slack}"
    excess = None
    if solve:
        cost = dist[rows, ass].sum()
        r, c = linear_sum_assignment(dist)
        opt = dist[r, c].sum()
        # two float64 sums of n terms <= dist.max(): each within n * 2^-53 of n * dist.max()
        assert cost >= opt - 2 * n * n * 2.0 ** -53 * dist.max()
        assert cost <= opt + n * (eps + slack), f"cost {cost} above OPT {opt} + n*eps {n * eps}"
        excess = (cost - opt) / (n * eps)
    return EpsOptimal(excess, float(gap.max()), big, slack)
