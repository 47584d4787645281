"""Density-aware Chamfer checks that need no GPU: the numpy restatement of
tests/dcd_restated.py against a brute-force double loop, central differences
and identities; the two conditions that hold the GPU test's bounds; the
library's exports, constants, validation and workspace size; loss/dcd_loss.py
without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dcd_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
# the comparison's shapes that a CPU test can afford (the two largest only pass through the oracle once, on the GPU run)
SMALL = [s for s in R.SHAPES if s[0] * s[1] * s[2] <= 1 << 22]


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(7, 5), (12, 9), (1, 4)])
def test_restatement_is_the_brute_force_double_loop(oracle, n, m):
    x, y = R.make_clouds(2, n, m, seed=1)
    d1, d2, i1, i2 = oracle.chamfer_forward(x, y)
    alpha = R.median_alpha(d1, d2)
    for lam in R.LAMBDAS + [2.0]:
        for non_reg in (False, True):
            res = R.evaluate(d1, d2, i1, i2, alpha, lam, non_reg)
            for bi in range(2):
                want, (b1, b2, j1, j2) = R.brute_loss(x[bi], y[bi], alpha, lam, non_reg)
                assert np.array_equal(j1, i1[bi]) and np.array_equal(j2, i2[bi])
                assert np.abs(b1 - d1[bi]).max() <= 4 * R.U32 * 3 and np.abs(b2 - d2[bi]).max() <= 4 * R.U32 * 3
                # the float32 distances against the float64 ones: alpha |delta d| of a term
                assert abs(res["loss"][bi] - want) <= float(alpha) * 12 * R.U32 + 1e-12, (lam, non_reg, bi)
                assert 1e-3 < abs(want) < 4.0  # r = 4 at (1, 4): a term may be negative
            assert np.array_equal(res["c1"], np.stack([np.bincount(r, minlength=n) for r in i2]))
            assert res["c1"].sum() == 2 * m and res["c2"].sum() == 2 * n


def _loss64(x, y, alpha, lam, non_reg):
    """float64 loss of one element from the points, with its argmins."""
    dd = ((x[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    i1, i2 = dd.argmin(axis=1), dd.argmin(axis=0)
    res = R.evaluate(dd.min(axis=1)[None], dd.min(axis=0)[None], i1[None], i2[None], alpha, lam, non_reg)
    return res, i1, i2


def test_gradient_is_the_central_difference():
    x, y = (c[0].astype(np.float64) for c in R.make_clouds(1, 20, 13, seed=2))
    lam, non_reg = 0.5, True
    res, i1, i2 = _loss64(x, y, 1.0, lam, non_reg)
    alpha = R.median_alpha(res["a1"], res["a2"])  # a = d at alpha 1
    res, i1, i2 = _loss64(x, y, alpha, lam, non_reg)
    gx, gy = R.gradients(x[None], y[None], i1[None], i2[None], res["gd1"], res["gd2"])
    h = 1e-6
    checked = 0
    for cloud, g in ((0, gx[0]), (1, gy[0])):
        for i in range(len(g)):
            for c in range(3):
                vals = []
                for sign in (1.0, -1.0):
                    pts = [x.copy(), y.copy()]
                    pts[cloud][i, c] += sign * h
                    moved, j1, j2 = _loss64(pts[0], pts[1], alpha, lam, non_reg)
                    assert np.array_equal(j1, i1) and np.array_equal(j2, i2)  # the step leaves every argmin
                    vals.append(moved["loss"][0])
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - g[i, c]) <= 1e-6 * max(abs(g[i, c]), 1e-3), (cloud, i, c, fd, g[i, c])
                checked += 1
    assert checked == 3 * 33 and np.abs(gx).max() > 1e-3 and np.abs(gy).max() > 1e-3


def test_identities(oracle):
    x, y = R.make_clouds(2, 100, 33, seed=3)
    d1, d2, i1, i2 = oracle.chamfer_forward(x, y)
    alpha = R.median_alpha(d1, d2)
    # lambda = 0: the plain exponential Chamfer, no count anywhere
    res = R.evaluate(d1, d2, i1, i2, alpha, 0.0, False)
    a = float(alpha)
    want = 0.5 * ((1 - np.exp(-a * d1.astype(np.float64)) * (100 / 33) / (1 + R.EPS)).mean(axis=1)
                  + (1 - np.exp(-a * d2.astype(np.float64)) * (33 / 100) / (1 + R.EPS)).mean(axis=1))
    assert np.abs(res["loss"] - want).max() <= 1e-14
    # n = m = 1
    p, q = R.make_clouds(3, 1, 1, seed=3)
    e1, e2, j1, j2 = oracle.chamfer_forward(p, q)
    assert not j1.any() and not j2.any() and np.array_equal(e1, e2)
    res = R.evaluate(e1, e2, j1, j2, 2.0, 1.0, False)
    assert np.abs(res["loss"] - (1 - np.exp(-2.0 * e1[:, 0].astype(np.float64)) / (1 + R.EPS))).max() <= 1e-15
    assert np.array_equal(res["c1"], np.ones((3, 1))) and np.array_equal(res["c2"], np.ones((3, 1)))
    # y = x: every distance 0, every count 1, every term 1 - 1 / (1 + 1e-6)
    d1, d2, i1, i2 = oracle.chamfer_forward(x, x)
    assert not d1.any() and np.array_equal(i1[0], np.arange(100))
    res = R.evaluate(d1, d2, i1, i2, 1000.0, 1.0, False)
    assert np.abs(res["loss"] - R.EPS / (1 + R.EPS)).max() <= 1e-15 and 0.9e-6 < res["loss"][0] < 1.1e-6
    # all of x at one point: every point of y has x[0] as its neighbour -- one count of m
    one = np.repeat(x[:, :1], 100, axis=1)
    d1, d2, i1, i2 = oracle.chamfer_forward(one, y)
    res = R.evaluate(d1, d2, i1, i2, alpha, 1.0, False)
    assert not i2.any() and np.array_equal(res["c1"][:, 0], [33, 33]) and not res["c1"][:, 1:].any()
    assert len(np.unique(i1[0])) == 1 and res["c2"][0].max() == 100


# ---------------------------------------------------------------------------
# the two conditions on the bounds
# ---------------------------------------------------------------------------
def _ratios(res, other, alpha, lam, n, m):
    """largest error / bound of `other` against `res` for (loss, cd, gd1, gd2); 0 / 0 counts as 0."""
    out = []
    for bound, key in zip(R.bounds(res, alpha, lam, n, m), ("loss", "cd", "gd1", "gd2")):
        err = np.abs(np.asarray(other[key], np.float64) - res[key])
        out.append(float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)))))
    return out


def test_float32_restatement_is_within_the_bounds():
    """Condition (a): the pinned chain evaluated in float32 by numpy against
    the float64 restatement, on the shapes of the GPU comparison."""
    worst = np.zeros(4)
    for b, n, m in SMALL:
        x, y, d1, d2, i1, i2, alpha = R.forward(b, n, m)
        for lam in R.LAMBDAS:
            for non_reg in (False, True):
                res = R.evaluate(d1, d2, i1, i2, alpha, lam, non_reg)
                f32 = R.evaluate(d1, d2, i1, i2, alpha, lam, non_reg, dtype=np.float32)
                figures = _ratios(res, f32, alpha, lam, n, m)
                worst = np.maximum(worst, figures)
                assert max(figures) <= 1.0, ((b, n, m, lam, non_reg), figures)
    print("float32 evaluation, largest error / bound: loss %.3g cd %.3g graddist1 %.3g graddist2 %.3g" % tuple(worst))


def test_modelled_defects_leave_the_bounds():
    """Condition (b), on the restatement and the GPU test's inputs, not on any
    kernel: each defect moves the loss or a graddist by more than ten bounds
    on the cases that exercise it."""
    checked = {k: 0 for k in ("swap_r", "cross_counts", "drop_tail", "ignore_lambda", "ignore_non_reg")}
    for b, n, m in SMALL:
        if n == 1 and m == 1:
            continue
        x, y, d1, d2, i1, i2, alpha = R.forward(b, n, m)
        for lam in R.LAMBDAS:
            for non_reg in (False, True):
                res = R.evaluate(d1, d2, i1, i2, alpha, lam, non_reg)
                for defect in checked:
                    exercised = {"swap_r": n != m and not non_reg, "cross_counts": lam != 0,
                                 "drop_tail": lam != 0 and (n % 64 != 0 or m % 64 != 0),
                                 "ignore_lambda": lam == 0.5, "ignore_non_reg": n != m and non_reg}[defect]
                    if not exercised:
                        continue
                    bad = R.evaluate(d1, d2, i1, i2, alpha, lam, non_reg, defect=defect)
                    figures = _ratios(res, bad, alpha, lam, n, m)
                    assert max(figures[0], figures[2], figures[3]) > 10.0, ((b, n, m, lam, non_reg), defect, figures)
                    checked[defect] += 1
    assert min(checked.values()) >= 5, checked


# ---------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------
def test_library_exports_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_dcd_workspace_bytes", "pcm_dcd_loss"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    assert int(re.search(r"#define\s+PCM_DCD_MAX_POINTS\s+(\d+)", src).group(1)) == pcm_hip.DCD_MAX_POINTS
    assert pcm_hip.DCD_MAX_POINTS == R.MAX_POINTS == 16384
    # integer LDS atomics only, no waiting between workgroups; the term's order needs contraction off
    hip = open(os.path.join(CSRC, "dcd.hip")).read()
    lines = [ln.split("//", 1)[0] for ln in hip.splitlines()]
    atomics = [ln for ln in lines if "atomic" in ln.lower()]
    assert len(atomics) == 2 and all("atomicAdd(&hist" in ln and ", 1)" in ln for ln in atomics)
    assert not [ln for ln in lines if "s_sleep" in ln]
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()


def test_workspace_size():
    import pcm_hip
    lib = pcm_hip.load_library()
    need = lib.pcm_dcd_workspace_bytes
    for args in ((0, 4, 4), (-1, 4, 4), (2, 0, 4), (2, 4, 0), (2, -4, 4)):
        assert need(*args) == 0
    # distances, argmins and graddists of both directions, and a gradient each
    assert need(2, 300, 1025) >= 2 * 1325 * (3 * 4 + 3 * 4)
    last = 0
    for b in (1, 2, 3, 8, 16, 17, 32):  # monotone in b, through the grid forward's threshold (b = 16)
        for n, m in ((1024, 1024), (4096, 4096), (16384, 16384), (100, 33)):
            assert need(b + 1, n, m) > need(b, n, m)
            assert need(b, n, m) >= lib.pcm_chamfer_forward_ws_bytes(b, n, m) + b * (n + m) * 24
        assert need(b, 4096, 4096) > last
        last = need(b, 4096, 4096)
    assert lib.pcm_chamfer_forward_ws_bytes(16, 4096, 4096) > 0 and lib.pcm_chamfer_forward_ws_bytes(1, 16384, 16384) > 0
    assert pcm_hip.dcd_workspace_bytes(2, 300, 1025) == need(2, 300, 1025)


def _host_pointer():
    # a non-null, 16-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_dcd_loss_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 44
    nan, inf = float("nan"), float("inf")

    def call(b=2, n=8, m=9, l1=0, l2=0, alpha=10.0, lam=1.0, non_reg=0, x=one, y=one, loss=one, cd=null, g1=null,
             g2=null, c1=null, c2=null, gd1=null, gd2=null, ws=one, ws_bytes=big):
        return lib.pcm_dcd_loss(x, y, b, n, m, l1, l2, alpha, lam, non_reg, loss, cd, g1, g2, c1, c2, gd1, gd2, ws,
                                ws_bytes, null)

    assert call(b=-1) == INVALID and call(n=-8) == INVALID and call(m=-1) == INVALID
    assert call(l1=2) == INVALID and call(l2=-1) == INVALID
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert call(alpha=bad) == INVALID, bad
    for bad in (-0.5, nan, inf):
        assert call(lam=bad) == INVALID, bad
    assert call(b=0, alpha=0.0) == INVALID and call(b=0, l1=3) == INVALID and call(b=0, lam=-1.0) == INVALID  # before b == 0
    # then b == 0 is a no-op, also with null pointers
    assert call(b=0) == OK
    assert call(b=0, n=0, m=0, x=null, y=null, loss=null, ws=null, ws_bytes=0) == OK
    assert call(n=0) == INVALID and call(m=0) == INVALID
    assert call(x=null) == INVALID and call(y=null) == INVALID and call(loss=null) == INVALID
    assert call(n=pcm_hip.DCD_MAX_POINTS + 1) == UNSUPPORTED and call(m=pcm_hip.DCD_MAX_POINTS + 1) == UNSUPPORTED
    assert call(n=0, m=pcm_hip.DCD_MAX_POINTS + 1) == INVALID  # invalid comes first
    assert call(x=null, n=pcm_hip.DCD_MAX_POINTS + 1) == INVALID
    # the limits themselves are taken
    assert call(n=pcm_hip.DCD_MAX_POINTS, m=pcm_hip.DCD_MAX_POINTS, ws=null) == WORKSPACE
    assert call(ws=null) == WORKSPACE
    assert call(ws_bytes=lib.pcm_dcd_workspace_bytes(2, 8, 9) - 1) == WORKSPACE
    assert call(g1=one, g2=one, cd=one, ws_bytes=lib.pcm_dcd_workspace_bytes(2, 8, 9) - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(one.value + 8)) == INVALID  # not 16-byte aligned
    assert call(ws=null, ws_bytes=0, n=-1) == INVALID
    assert call(lam=0.0, ws=null) == WORKSPACE and call(lam=2.5, non_reg=1, ws=null) == WORKSPACE  # both are valid
    del keep


def test_module_imports_without_a_device_and_raises():
    import dcd_loss
    import loss
    import pcm_hip
    doc = " ".join(dcd_loss.__doc__.split())
    assert "stated from the published source, not verified against it" in doc
    assert "2048 points or more" in doc and "smaller alpha" in doc and "detached" in doc
    L = dcd_loss.DCDLoss()
    assert (L.alpha, L.n_lambda, L.non_reg) == (1000.0, 1.0, False)
    x, y = torch.rand(2, 10, 3), torch.rand(2, 12, 3)
    with pytest.raises(RuntimeError):  # no CPU path
        L(x, y)
    with pytest.raises(RuntimeError):
        dcd_loss.calc_dcd(x, y)
    with pytest.raises(RuntimeError):
        dcd_loss.calc_dcd(x, y, alpha=40, n_lambda=0.5, return_raw=True, non_reg=True)
    with pytest.raises(TypeError):
        L(x.double(), y.double())
    with pytest.raises(TypeError):
        dcd_loss.calc_dcd(x.half(), y.half())
    with pytest.raises(ValueError):
        L(x[:, :, :2], y)
    with pytest.raises(ValueError):
        L(x, y[:1])
    for bad in (dict(alpha=0), dict(alpha=-1), dict(alpha=float("nan")), dict(n_lambda=-1), dict(n_lambda=float("inf"))):
        with pytest.raises(ValueError):
            dcd_loss.DCDLoss(**bad)
        with pytest.raises(ValueError):
            dcd_loss.calc_dcd(x, y, **bad)
    with pytest.raises(RuntimeError):
        loss.Loss().get_dcd_loss(x, y)
    with pytest.raises(RuntimeError):
        loss.Loss().get_dcd_loss(x.transpose(1, 2).contiguous().transpose(2, 1), y, alpha=50, n_lambda=0.5)
    with pytest.raises(RuntimeError):  # the binding itself
        pcm_hip.dcd_loss(x, 0, y, 0, 1000.0, 1.0, False, torch.empty(2))
