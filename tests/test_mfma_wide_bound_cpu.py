"""The error bound of the wide matrix-core Chamfer screen (fused variant 20,
csrc/chamfer_filt.hip filt_forward_mfma<.., true>), restated in numpy.

The screen value a(q, t) = w + u.q' (u = -2 t', w = |t'|^2, both formed in
fp32 from the centred clouds) is summed over 21 K slots of exact bf16 x bf16
products: per dimension uh qh, uh qm, um qh, uh ql, ul qh, um qm (K 6d..6d+5),
then wh, wm, wl against 1 (K 18..20).  The wide loop sums K 0..15 in a first
v_mfma_f32_32x32x16_bf16 onto zero and adds K 16..20 (and eleven zero slots)
in a second one onto that result: 20 fp32 additions, as in the narrow loop,
whose order and rounding inside the instruction are not specified.  Checked
here for several orders, rounding to nearest and truncating: on random and
large-radius clouds |screen - exact| <= 80 u (R + |q'|)^2, u = 2^-24, the E
the proof uses (kFiltU80), where exact is |t'|^2 - 2 t'.q' in float64 and
R = max |t'|.
"""
import numpy as np
import pytest

from test_bf16_split_cpu import split3

U = 2.0 ** -24


def _terms(q, t):
    """fp32 [nq, nt, 21]: the K slots' products, each exact in fp32."""
    c = (q.sum(axis=0, dtype=np.float32) / np.float32(q.shape[0])).astype(np.float32)
    qc, tc = (q - c).astype(np.float32), (t - c).astype(np.float32)
    x, y, z = tc[:, 0], tc[:, 1], tc[:, 2]
    w = (z * z + (y * y + x * x).astype(np.float32)).astype(np.float32)
    u = (np.float32(-2.0) * tc).astype(np.float32)  # exact
    slots = []
    for d in range(3):
        uh, um, ul, _, _ = split3(u[:, d])
        qh, qm, ql, _, _ = split3(qc[:, d])
        for a, b in ((uh, qh), (uh, qm), (um, qh), (uh, ql), (ul, qh), (um, qm)):
            p64 = a.astype(np.float64)[None, :] * b.astype(np.float64)[:, None]
            p = p64.astype(np.float32)
            assert np.array_equal(p.astype(np.float64), p64)  # 8-bit x 8-bit: exact
            slots.append(p)
    for part in split3(w)[:3]:
        slots.append(np.broadcast_to(part[None, :], (q.shape[0], t.shape[0])))
    exact = (tc.astype(np.float64) ** 2).sum(axis=1)[None, :] - 2.0 * qc.astype(np.float64) @ tc.astype(np.float64).T
    r = np.sqrt((tc.astype(np.float64) ** 2).sum(axis=1).max())
    qn = np.sqrt((qc.astype(np.float64) ** 2).sum(axis=1))
    return np.stack(slots, axis=-1), exact, r, qn


def _add_rn(a, b):
    return (a + b).astype(np.float32)


def _add_rz(a, b):
    """fp32 addition rounded toward zero (through float64, exact for operands
    less than 2^29 apart, as the slots of one sum are)."""
    s = a.astype(np.float64) + b.astype(np.float64)
    r = s.astype(np.float32)
    over = np.abs(r.astype(np.float64)) > np.abs(s)
    return np.where(over, np.nextafter(r, np.float32(0)), r).astype(np.float32)


def _chain(v, order, add):
    s = v[..., order[0]]
    for k in order[1:]:
        s = add(s, v[..., k])
    return s


def _tree(v, add):
    parts = [v[..., k] for k in range(v.shape[-1])]
    while len(parts) > 1:
        nxt = [add(parts[i], parts[i + 1]) for i in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        parts = nxt
    return parts[0]


def _blocks4(v, add):
    """Four running sums over K mod 4, then their sum."""
    acc = [_chain(v[..., j::4], list(range(v[..., j::4].shape[-1])), add) for j in range(4)]
    return add(add(acc[0], acc[1]), add(acc[2], acc[3]))


def _screens(terms):
    """The wide screen for several orders of the two MFMAs' sums: K 0..15
    first (onto an exact zero), then K 16..20 added to that result."""
    lo, hi = terms[..., :16], terms[..., 16:]
    for add in (_add_rn, _add_rz):
        for name, first in (("ascending", _chain(lo, list(range(16)), add)),
                            ("descending", _chain(lo, list(range(15, -1, -1)), add)),
                            ("tree", _tree(lo, add)),
                            ("blocks of 4", _blocks4(lo, add))):
            # (the first MFMA's zero C adds nothing in any order.)  The second
            # MFMA: C first and then its slots, its slots first and then C, as a tree
            yield f"{name}, then C + K16..20 ({add.__name__})", _chain(
                np.concatenate([first[..., None], hi], axis=-1), list(range(6)), add)
            yield f"{name}, then K20..16 + C ({add.__name__})", add(_chain(hi, [4, 3, 2, 1, 0], add), first)
            yield f"{name}, then tree(K16..20) + C ({add.__name__})", add(_tree(hi, add), first)


def _clouds(kind):
    rng = np.random.default_rng({"unit": 1, "kilo offset": 2, "far targets": 3, "shell": 4}[kind])
    nq, nt = 96, 1024
    if kind == "unit":
        q, t = rng.random((nq, 3)), rng.random((nt, 3))
    elif kind == "kilo offset":  # the GPU tests' scale and offset
        q, t = rng.random((nq, 3)) * 1e3 + 100.0, rng.random((nt, 3)) * 1e3 + 100.0
    elif kind == "far targets":  # R >> |q'|: w and u.q' cancel to differences far below either
        q = rng.random((nq, 3)) * 0.01
        t = rng.standard_normal((nt, 3))
        t = 1e3 * t / np.linalg.norm(t, axis=1, keepdims=True) + rng.random((nt, 3)) * 0.01
    else:  # queries and targets on one large shell around the centre
        q = rng.standard_normal((nq, 3))
        q = 5e2 * q / np.linalg.norm(q, axis=1, keepdims=True)
        t = rng.standard_normal((nt, 3))
        t = 5e2 * t / np.linalg.norm(t, axis=1, keepdims=True)
    return q.astype(np.float32), t.astype(np.float32)


@pytest.mark.parametrize("kind", ["unit", "kilo offset", "far targets", "shell"])
def test_wide_screen_within_80u(kind):
    q, t = _clouds(kind)
    terms, exact, r, qn = _terms(q, t)
    bound = 80.0 * U * (r + qn[:, None]) ** 2
    n = 0
    for name, screen in _screens(terms):
        err = np.abs(screen.astype(np.float64) - exact)
        worst = (err / bound).max()
        assert np.all(err <= bound), f"{kind}, {name}: {worst:.3f} of the bound"
        n += 1
    assert n == 24
