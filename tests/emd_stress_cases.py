"""EMD auction inputs outside the unit cube and on degenerate geometry.

Shared by tests/test_emd_stress_cpu.py (which keeps the oracle honest on these
inputs: convergence, eps-complementary slackness, cost against an exact solver)
and tests/test_emd_stress_gpu.py (HIP kernels against the oracle, bit for bit,
and against the auction's guarantee without the oracle).  Everything is seeded
numpy, so both see the same bits.

Every other EMD input of the suite is uniform in [0,1)^3.  The families here
move what csrc/emd.hip's pruning bounds were derived for:
  * scale: values 3 - ||x - y|| - price far from 3 (|K*'| dominates the fast
    scan's bound T), prices whose float32 ulp nears eps, increments inside the
    1e-6 GetMax window (scale_1e-4);
  * offset: cancellation inside the squared distance; centred clouds are what
    real data looks like;
  * plane / line / lattice: masses of exactly equal keys (select_cache's
    bisection cannot separate them);
  * identical / collapsed / clustered / bimodal / far target: the seed-time
    reserve's dK and th logic and its fall-back.
Non-finite coordinates and magnitudes at which a squared distance overflows
float32 are outside pcm_emd_forward's contract (include/pcm.h) and not here.
"""
import numpy as np

SHORT_ITERS = 300
CONVERGE_ITERS = 3000


def base(seed, b, n):
    g = np.random.default_rng(seed)
    return g.random((b, n, 3), dtype=np.float32), g.random((b, n, 3), dtype=np.float32)


def _f32(*v):
    return np.array(v, dtype=np.float32)


def _scaled(s):
    return lambda a, c: (a * np.float32(s), c * np.float32(s))


def _shifted(*off):
    return lambda a, c: (a + _f32(*off), c + _f32(*off))


def _plane(a, c):
    a[..., 2] = 0.5
    c[..., 2] = 0.5
    return a, c


def _line(a, c):
    a[..., 1:] = 0
    c[..., 1:] = 0
    return a, c


def _lattice_half_shift(a, c):
    # the 8 x 8 x (16 n / 1024) integer lattice / 16 (exact in float32); bidders
    # are the lattice permuted, targets the lattice shifted by half a cell along
    # x: every bidder with x > 0 has two exactly equidistant nearest targets
    b, n, _ = a.shape
    i, j, k = np.indices((8, 8, 16 * n // 1024))
    g = (np.stack([i, j, k], -1).reshape(n, 3) / 16).astype(np.float32)
    perm = np.random.default_rng(3)
    a = np.stack([g[perm.permutation(n)] for _ in range(b)])
    c = np.broadcast_to(g + _f32(1 / 32, 0, 0), (b, n, 3)).copy()
    return a, c


def _identical(a, c):
    return a, a.copy()


def _bimodal(a, c):
    n = a.shape[1]
    a[:, : n // 2] += _f32(1000, 0, 0)
    c[:, n // 2:] += _f32(1000, 0, 0)
    return a, c


def _collapsed_targets(a, c):
    c[:] = _f32(0.3, 0.6, 0.9)
    return a, c


_CENTRES = _f32((0.2, 0.2, 0.2), (0.8, 0.3, 0.5), (0.4, 0.9, 0.1), (0.6, 0.5, 0.8))


def _clustered_targets(a, c):
    n = a.shape[1]
    return a, _CENTRES[np.arange(n) % 4] + np.float32(1e-3) * c


def _far_target(a, c):
    c[:, 7] = _f32(30, -30, 30)
    return a, c


def _far_cloud(a, c):
    # every value is near -1e4, where a float32 ulp (1e-3) is about the spacing
    # of the 1024 values of a bidder: exact ties in mass at large |value|, which
    # the lattice (values near 3) and the scaled clouds (no ties) do not have.
    # The oracle still has 504 bidders after 3000 iterations (prices rose 11
    # times): held to the oracle only.
    return a, c + _f32(1e4, 0, 0)


# name -> (construction from `a, c = base(...)`, eps)
CASES = {
    "scale_1e-4": (_scaled(1e-4), 5e-6),
    "scale_1e3": (_scaled(1e3), 50.0),
    "scale_1e5": (_scaled(1e5), 5e3),
    "small_scale_big_eps": (_scaled(1e-3), 0.05),
    "offset_100": (_shifted(100, 100, 100), 0.05),
    "mixed_offset": (_shifted(1000, -1000, 0), 0.05),
    "centred": (_shifted(-0.5, -0.5, -0.5), 0.05),
    "plane": (_plane, 0.05),
    "line": (_line, 0.05),
    "lattice_half_shift": (_lattice_half_shift, 0.05),
    "identical": (_identical, 0.05),
    "bimodal": (_bimodal, 0.05),
    "collapsed_targets": (_collapsed_targets, 0.05),
    "clustered_targets": (_clustered_targets, 0.05),
    "far_target": (_far_target, 0.05),
    "far_cloud": (_far_cloud, 0.05),
}

# n = 2048 is the largest LDS-state form, n = 4096 the workspace-state, staged form
SWEPT = ("scale_1e-4", "scale_1e3", "lattice_half_shift", "bimodal")

# (name, n) that are held to the oracle only: the oracle's auction still has
# bidders at iteration CONVERGE_ITERS (one, one and 504), so the result is not
# a bijection
NOT_CONVERGING = (("far_target", 1024), ("scale_1e-4", 4096), ("far_cloud", 1024))

# the global-memory cloud form, a few iterations, oracle parity only
LARGE = ("scale_1e3", 16384, 30)

ENTRIES = [(name, 1024) for name in CASES] + [(name, n) for n in (2048, 4096) for name in SWEPT]
CONVERGING = [e for e in ENTRIES if e not in NOT_CONVERGING]


def clouds(name, n, b=1):
    """The case's two float32 [b, n, 3] clouds and its eps.  Batch element i is
    built from seed 100 + n + 1000 i, so no two elements repeat."""
    assert b == 1 or name != "lattice_half_shift"  # the lattice has no seed: a repeat
    make, eps = CASES[name]
    parts = [make(*base(100 + n + 1000 * i, 1, n)) for i in range(b)]
    a = np.ascontiguousarray(np.concatenate([p[0] for p in parts]), dtype=np.float32)
    c = np.ascontiguousarray(np.concatenate([p[1] for p in parts]), dtype=np.float32)
    return a, c, eps


def entry_id(entry):
    return f"{entry[0]}-n{entry[1]}"
