"""The three-way bf16 split behind the matrix-core Chamfer screen
(csrc/chamfer_filt.hip split3x2), restated in numpy: each level is the
round-to-nearest-even bf16 of the remainder of the levels above.

Checked here, on random and adversarial inputs: every remainder is exact in
fp32, the three parts miss v by at most 2^-24 |v|, and the product terms the
screen drops (um*ql, ul*qm, ul*ql and the split's own residues) stay within
the 4.01 u |u q| of the file header (u = 2^-24).
"""
import numpy as np

U = 2.0 ** -24


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split3(v):
    v = np.asarray(v, dtype=np.float32)
    h = bf16_rne(v)
    r1 = (v - h).astype(np.float32)
    m = bf16_rne(r1)
    r2 = (r1 - m).astype(np.float32)
    return h, m, bf16_rne(r2), r1, r2


def _inputs():
    rng = np.random.default_rng(20)
    parts = []
    for scale in (1.0, 1e-30, 3e19):  # the GPU tests' coordinate scales
        parts.append((rng.random(40000) * 2 - 1) * scale)
        parts.append(rng.standard_normal(20000) * 10 * scale)
    v = np.concatenate(parts).astype(np.float32)
    # powers of two and their neighbours
    p2 = np.ldexp(1.0, np.arange(-100, 64)).astype(np.float32)
    near = [p2, -p2, np.nextafter(p2, np.float32(0)), np.nextafter(p2, np.float32(np.inf))]
    # one fp32 ulp either side of a bf16 tie (and the ties), at the first and second level
    hi = rng.integers(0x0800, 0x7000, 20000).astype(np.uint32) << 16  # exponents well inside the normal range
    ties = []
    for low in (0x8000, 0x7FFF, 0x8001, 0x0080, 0x007F, 0x0081, 0x8080, 0x807F, 0x8081, 0x7F80, 0xFFFF, 0x0001):
        ties.append((hi | np.uint32(low)).view(np.float32))
    v = np.concatenate([v] + near + ties + [-t for t in ties]).astype(np.float32)
    return v[np.abs(v) < 2.0 ** 100]  # (no part rounds up to inf)


# Below about 2^-109 the lower parts of a value are subnormal bf16, whose
# spacing is 2^-133: a part's rounding error is then absolute, at most DELTA,
# instead of relative.  The proof's absolute 2^-100 covers what that adds to
# the screened value (checked in the product test).
DELTA = 2.0 ** -134


def test_remainders_are_exact_and_parts_sum_to_v():
    v = _inputs()
    assert np.count_nonzero(np.abs(v) < 1e-29) > 50000  # the 1e-30-scale inputs are in
    assert np.count_nonzero((v != 0) & (np.abs(v) < 2.0 ** -109)) > 0  # and some have subnormal parts
    h, m, l, r1, r2 = split3(v)
    v64, h64, m64, l64 = (a.astype(np.float64) for a in (v, h, m, l))
    assert np.array_equal(r1.astype(np.float64), v64 - h64)
    assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - m64)
    for part in (h, m, l):  # each part is a bf16: low 16 bits clear
        assert not np.any(part.view(np.uint32) & 0xFFFF)
    err = np.abs(v64 - (h64 + m64 + l64))
    assert np.all(err <= np.maximum(U * np.abs(v64), DELTA))
    normal = np.abs(v64) >= 2.0 ** -109  # every part a normal bf16 (or zero): the relative bound alone
    assert np.all(err[normal] <= U * np.abs(v64[normal]))


def test_dropped_product_terms_within_header_bound():
    v = _inputs()
    rng = np.random.default_rng(21)
    u = v
    for q in (rng.permutation(v), v, -v[::-1]):  # products of every pairing of scales (all finite in float64)
        uh, um, ul, _, _ = (a.astype(np.float64) for a in split3(u))
        qh, qm, ql, _, _ = (a.astype(np.float64) for a in split3(q))
        # the six K slots per dimension: uh qh, uh qm, um qh, uh ql, ul qh, um qm
        # (8-bit by 8-bit products and their sum are exact in float64)
        kept = uh * qh + uh * qm + um * qh + uh * ql + ul * qh + um * qm
        u64, q64 = u.astype(np.float64), q.astype(np.float64)
        exact = u64 * q64
        err = np.abs(exact - kept)
        # every part and residue is off its relative bound by at most DELTA, and
        # each meets a factor no larger than the other operand (four such terms)
        s = np.abs(u64) + np.abs(q64)
        allow = 4.0 * DELTA * (s + DELTA)
        assert np.all(err <= 4.01 * U * np.abs(exact) + allow)
        normal = (np.abs(u64) >= 2.0 ** -109) & (np.abs(q64) >= 2.0 ** -109)
        assert np.all(err[normal] <= 4.01 * U * np.abs(exact[normal]))
        # three dimensions of that allowance fit the proof's budget: its absolute
        # 2^-100, or one u (R + |q'|)^2 of the slack between the 59u it derives
        # and the 80u it uses (|u| + |q| <= 2 (R + |q'|))
        assert np.all(3.0 * allow <= 2.0 ** -100 + U * s * s / 4.0)
