"""The inputs on which the oracle is pinned to the reference's own kernels.

Shared by tests/test_oracle_reference_cpu.py (oracle vs. the host build of the
reference's kernels, oracle/ref_build.py) and tests/golden/make_ref_kernels_golden.py
(which records a subset with the reference's outputs for the GPU suite).
Everything is seeded numpy, so both see the same bits.
"""
import numpy as np

import emd_stress_cases as S


def uniform_clouds(seed, b, n):
    g = np.random.default_rng(seed)
    return g.random((b, n, 3), dtype=np.float32), g.random((b, n, 3), dtype=np.float32)


def exact_tie_clouds(seed, b, n):
    """tests/test_emd_gpu.py::test_emd_exact_ties_follow_reference_order restated
    in numpy: a quarter of the targets duplicated, an eighth of the bidders
    sitting exactly on duplicated targets -> exact ties at the best value."""
    g = np.random.default_rng(seed)
    a = g.random((b, n, 3), dtype=np.float32)
    c = g.random((b, n, 3), dtype=np.float32)
    src = g.permutation(n)[: n // 4]
    dst = g.permutation(n)[: n // 4]
    c[:, dst] = c[:, src]
    on = g.permutation(n)[: n // 8]
    a[:, on] = c[:, dst[: n // 8]]
    return a, c


def chamfer_clouds(seed, b, n, m, nan_targets=(), inf_targets=(), nan_queries=()):
    """Uniform clouds, a quarter of the targets duplicated (exact distance ties),
    then non-finite coordinates at the named points of every batch element."""
    g = np.random.default_rng(seed)
    a = g.random((b, n, 3), dtype=np.float32)
    c = g.random((b, m, 3), dtype=np.float32)
    dst = g.permutation(m)[: m // 4]
    src = g.permutation(m)[: m // 4]
    c[:, dst] = c[:, src]
    for k in nan_targets:
        c[:, k, 1] = np.nan
    for k in inf_targets:
        c[:, k, 0] = np.inf
    for k in nan_queries:
        a[:, k, 2] = np.nan
    return a, c


# name -> (clouds, eps, iters, race_free, converged)
#   race_free: the reference's output must not depend on the thread schedule
#              (ascending == descending); the others need the descending
#              (lowest index wins GetMax) schedule to be deterministic at all.
#   converged: no bidder is left in the last iteration, so the reference's racy
#              last-iteration `price +=` (emd_cuda.cu:201-211) never runs and the
#              price can be compared in full.
EMD_CASES = {
    "b2_n1024_eps005": (lambda: uniform_clouds(0, 2, 1024), 0.005, 50, True, False),
    # stands in for "B=1, N=1024, eps 0.05, 1500 iterations" (converges at
    # iteration 768, ~28 s per schedule in the emulator): eps 0.1 has no bidder
    # from iteration 245 on, 260 iterations take ~4 s per schedule
    "converged_n1024": (lambda: uniform_clouds(7, 1, 1024), 0.1, 260, True, True),
    "n3072": (lambda: uniform_clouds(3, 1, 3072), 0.05, 100, False, False),
    "exact_ties_n4096": (lambda: exact_tie_clouds(40, 1, 4096), 0.05, 60, False, False),
    # the oracle's double-precision GetMax window and its -1e9 start values away
    # from the unit cube (tests/emd_stress_cases.py, n = 1024).  Increments of
    # the two small-scale cases fall inside the 1e-6 window, where the schedule
    # picks the claimant: racy in the reference.  Values near -1e3 do not.
    "scale_1e-4": (lambda: S.clouds("scale_1e-4", 1024)[:2], S.CASES["scale_1e-4"][1], 60, False, False),
    "scale_1e3": (lambda: S.clouds("scale_1e3", 1024)[:2], S.CASES["scale_1e3"][1], 60, True, False),
    # no bidder from iteration 14 on
    "small_scale_big_eps": (lambda: S.clouds("small_scale_big_eps", 1024)[:2], S.CASES["small_scale_big_eps"][1],
                            40, False, True),
}

# name -> clouds.  The 512-point tile rules (chamfer3D.cu:36,79,121,126): a NaN
# at a tile's first point poisons that tile's best; tile 0's poisons the result.
CHAMFER_FORWARD_CASES = {
    # NaN at target 0 (every dist1 is NaN), at the starts of tiles 1 and 2, inf
    # at 700, a NaN query; M = 1300 leaves a 276-point last tile
    "nan_tiles_700x1300": lambda: chamfer_clouds(50, 2, 700, 1300, nan_targets=(0, 512, 1024),
                                                 inf_targets=(700,), nan_queries=(5,)),
    # M > 512 * 3 and the NaN at the first point of the fourth (64-point) tile
    "nan_tile3_300x1600": lambda: chamfer_clouds(51, 1, 300, 1600, nan_targets=(1536,)),
    "finite_500x900": lambda: chamfer_clouds(52, 1, 500, 900),
}


def graddist(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def bits(x):
    """float32 array -> its bit patterns (so NaNs and signed zeros compare)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
