"""Sinkhorn divergence checks that need no GPU: the schedule; the numpy
restatement of tests/sinkhorn_restated.py against torch float64 autograd,
against finite differences and against the properties of a divergence; the two
conditions that hold the GPU test's tolerances; the library's exports,
constants, validation and workspace size; loss/sinkhorn_loss.py without a
device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sinkhorn_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
NAN, INF = float("nan"), float("inf")
SQRT3 = math.sqrt(3.0)


# ---------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------
def test_schedule_is_the_published_list():
    import pcm_hip
    eps = pcm_hip.sinkhorn_schedule(0.05, 0.5, SQRT3)
    want = [3, 3, 0.75, 0.1875, 0.046875, 0.01171875, 0.0029296875, 0.0025]
    assert len(eps) == 8
    assert eps == pytest.approx(want, rel=1e-6)  # blur and the diameter are float32 arguments
    assert eps == pytest.approx(R.schedule(0.05, 0.5, SQRT3), rel=1e-13)
    assert eps[0] == float(np.float32(SQRT3)) ** 2 and eps[1] == pytest.approx(eps[0], rel=1e-15)  # the duplicate
    assert eps[-1] == float(np.float32(0.05)) ** 2  # ends in blur^2
    assert all(a >= b for a, b in zip(eps, eps[1:]))
    for blur, scaling in R.SETTINGS:
        assert pcm_hip.sinkhorn_schedule(blur, scaling, R.DIAMETER) == pytest.approx(
            R.schedule(blur, scaling, R.DIAMETER), rel=1e-13)
    assert [len(R.schedule(bl, sc, R.DIAMETER)) for bl, sc in R.SETTINGS] == [8, 10]
    # a blur at or above the diameter: eps_0 and blur^2 alone
    assert pcm_hip.sinkhorn_schedule(2.0, 0.5, 1.0) == [1.0, 4.0]


def test_schedule_count_and_capacity():
    import pcm_hip
    lib = pcm_hip.load_library()
    assert lib.pcm_sinkhorn_schedule(0.05, 0.5, SQRT3, None, 0) == 8  # the count alone
    buf = (ctypes.c_double * 8)(*([-1.0] * 8))
    assert lib.pcm_sinkhorn_schedule(0.05, 0.5, SQRT3, buf, 7) == 8 and list(buf) == [-1.0] * 8  # too short: untouched
    assert lib.pcm_sinkhorn_schedule(0.05, 0.5, SQRT3, buf, 8) == 8 and buf[7] == float(np.float32(0.05)) ** 2


def test_schedule_rejects_bad_arguments():
    import pcm_hip
    sched = pcm_hip.load_library().pcm_sinkhorn_schedule
    for bad in (0.0, -0.05, NAN, INF, -INF):
        assert sched(bad, 0.5, SQRT3, None, 0) == INVALID  # blur
        assert sched(0.05, 0.5, bad, None, 0) == INVALID  # diameter
    for bad in (0.0, 1.0, -0.5, 1.5, NAN, INF, -INF):
        assert sched(0.05, bad, SQRT3, None, 0) == INVALID  # scaling outside (0, 1)
    assert sched(1e-3, 0.99, SQRT3, None, 0) == UNSUPPORTED  # 744 entries
    assert len(R.schedule(1e-3, 0.99, SQRT3)) > R.MAX_STEPS
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.sinkhorn_schedule(0.05, 1.0, SQRT3)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.sinkhorn_schedule(1e-3, 0.99, SQRT3)


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _torch_extrapolation(x, y, averaged, eps):
    """The extrapolation step's loss in torch float64 with the averaged
    potentials and the column points detached (the envelope rule)."""
    f_ba, g_ab, f_aa, g_bb = (torch.from_numpy(v) for v in averaged)
    n, m = len(x), len(y)
    la, lb = -math.log(n), -math.log(m)

    def softmin(p, q, h):
        C = 0.5 * ((p[:, None, :] - q.detach()[None, :, :]) ** 2).sum(-1)
        return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)

    F_ba, F_aa = softmin(x, y, lb + g_ab / eps), softmin(x, x, la + f_aa / eps)
    G_ab, G_bb = softmin(y, x, la + f_ba / eps), softmin(y, y, lb + g_bb / eps)
    return (F_ba - F_aa).sum() / n + (G_ab - G_bb).sum() / m


@pytest.mark.parametrize("blur,scaling", R.SETTINGS)
def test_restated_gradients_equal_autograd(blur, scaling):
    x, y = R.make_clouds(1, 40, 56)
    eps = R.schedule(blur, scaling, R.DIAMETER)
    res = R.sinkhorn_one(x[0], y[0], eps)
    gx, gy = R.grads_from(res)
    tx = torch.from_numpy(res["x"]).requires_grad_(True)
    ty = torch.from_numpy(res["y"]).requires_grad_(True)
    loss = _torch_extrapolation(tx, ty, res["averaged"], eps[-1])
    loss.backward()
    assert abs(loss.item() - R.loss_from(res)) <= 1e-13
    assert np.abs(tx.grad.numpy() - gx).max() <= 1e-13 and np.abs(ty.grad.numpy() - gy).max() <= 1e-13
    assert np.abs(gx).max() > 1e-3 and np.abs(gy).max() > 1e-3


def test_restated_is_a_divergence():
    x, y = R.make_clouds(1, 40, 56)
    blur, scaling = R.SETTINGS[0]
    L, gx, gy, _ = R.restated_one(x[0], x[0], blur, scaling)
    assert abs(L) <= 1e-15 and np.abs(gx).max() <= 1e-15 and np.abs(gy).max() <= 1e-15  # x = y
    L, gx, gy, pots = R.restated_one(x[0], y[0], blur, scaling)
    assert L > 1e-2  # distinct clouds
    L2, hy, hx, pots2 = R.restated_one(y[0], x[0], blur, scaling)  # symmetric in the clouds
    assert abs(L2 - L) <= 1e-15 and np.abs(hx - gx).max() <= 1e-15 and np.abs(hy - gy).max() <= 1e-15
    assert np.abs(np.concatenate([pots2[56:], pots2[:56]]) - pots).max() <= 1e-15
    # unchanged by duplicating every point of a cloud
    L3, _, _, _ = R.restated_one(x[0], np.repeat(y[0], 2, axis=0), blur, scaling)
    assert abs(L3 - L) <= 1e-15
    L4, _, _, _ = R.restated_one(x[0], np.repeat(x[0], 2, axis=0), blur, scaling)
    assert abs(L4) <= 1e-15


def test_gradient_formula_is_the_converged_loss_s_derivative():
    """With the schedule extended by 300 entries of blur^2 the potentials have
    converged and the envelope-rule gradient equals central finite differences
    of the loss itself."""
    x, y = R.make_clouds(1, 40, 56)
    blur, scaling = R.SETTINGS[0]
    eps = R.schedule(blur, scaling, R.DIAMETER)
    eps = eps + [eps[-1]] * 300
    _, gx, gy, _ = R.restated_one(x[0], y[0], blur, scaling, eps_list=eps)
    h = 2.0 ** -12  # exact in float32 next to coordinates in [0, 1)
    for cloud, g, (i, c) in ((0, gx, (7, 0)), (0, gx, (31, 2)), (1, gy, (12, 1))):
        pts = [np.array(x[0]), np.array(y[0])]
        vals = []
        for sign in (1.0, -1.0):
            moved = [p.copy() for p in pts]
            moved[cloud][i, c] = np.float32(pts[cloud][i, c] + sign * h)
            assert float(moved[cloud][i, c]) - float(pts[cloud][i, c]) == sign * h
            vals.append(R.restated_one(moved[0], moved[1], blur, scaling, eps_list=eps)[0])
        fd = (vals[0] - vals[1]) / (2 * h)
        print(cloud, i, c, "finite difference %.6e formula %.6e" % (fd, g[i, c]))
        # a central difference is off by h^2 / 6 times the third derivative, which is at most of the order of
        # |g| / eps^2 at eps = blur^2 = 2.5e-3: 1.6e-3 |g|
        assert abs(fd - g[i, c]) <= 2e-3 * abs(g[i, c]) + 1e-9, (cloud, i, c, fd, g[i, c])
        assert abs(g[i, c]) > 1e-4


# ---------------------------------------------------------------------------
# the two conditions on the tolerances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("blur,scaling", R.SETTINGS)
def test_float32_restatement_is_within_a_quarter_of_the_tolerances(blur, scaling):
    """Condition (a): the kernel's steps in float32 (numpy's exp2 and log2 in
    place of the hardware's) against the float64 restatement, on every shape.
    Largest seen: loss 1.4e-8, normalised gradient 2.2e-6, potentials 1.0e-6."""
    for b, n, m in R.SHAPES:
        x, y = R.make_clouds(b, n, m)
        L, gx, gy, pots = R.restated(b, n, m, blur, scaling)
        for bi in range(b):
            L32, gx32, gy32, p32 = R.restated_one_f32(x[bi], y[bi], blur, scaling)
            eg = max(n * np.abs(gx32 - gx[bi]).max(), m * np.abs(gy32 - gy[bi]).max())
            figures = (abs(L32 - L[bi]) / R.TOL_LOSS, eg / R.TOL_GRAD, np.abs(p32 - pots[bi]).max() / R.TOL_POT)
            print((b, n, m), bi, "error / tolerance: loss %.3f grad %.3f pot %.3f" % figures)
            assert max(figures) <= 0.25, ((b, n, m), bi, figures)


def _moved(res_full, res_cut, n, m, skip_rows=None):
    """True when the defect moves the loss or the normalised gradient by more than ten tolerances (a result
    that is no longer finite counts as moved)."""
    dl = abs(R.loss_from(res_cut, skip_rows) - R.loss_from(res_full))
    if not dl <= 10 * R.TOL_LOSS:
        return True
    if res_cut["weights"] is None:
        return False
    (gx, gy), (hx, hy) = R.grads_from(res_full), R.grads_from(res_cut)
    return max(n * np.abs(hx - gx).max(), m * np.abs(hy - gy).max()) > 10 * R.TOL_GRAD


@pytest.mark.parametrize("blur,scaling", R.SETTINGS)
def test_gpu_test_inputs_show_the_modelled_defects(blur, scaling):
    """Condition (b), on the restatement and the inputs, not on any kernel: for
    every shape of the GPU test with n + m >= 128, each of three defects moves
    the float64 loss or the normalised gradient by more than ten times the
    tolerance -- a schedule entry left out (each of the last three: an early
    entry, the eps_0 duplicate above all, is below the loss's resolution once
    the later ones have run), the first min(TILE, c) columns of one cloud left
    out of the cross softmins, the first min(ROWS, c) rows of one cloud left out
    of the loss."""
    eps = R.schedule(blur, scaling, R.DIAMETER)
    checked = 0
    for b, n, m in R.SHAPES:
        if n + m < 128:
            continue
        x, y = R.make_clouds(b, n, m)
        full = R.sinkhorn_one(x[0], y[0], eps)
        for k in range(len(eps) - 3, len(eps)):
            assert _moved(full, R.sinkhorn_one(x[0], y[0], eps[:k] + eps[k + 1:]), n, m), ((b, n, m), "entry", k)
        for cloud, c in ((0, n), (1, m)):
            cut = R.sinkhorn_one(x[0], y[0], eps, skip_cols=(cloud, 0, min(R.TILE, c)))
            assert _moved(full, cut, n, m), ((b, n, m), "columns", cloud)
            assert _moved(full, full, n, m, skip_rows=(cloud, 0, min(R.ROWS, c))), ((b, n, m), "rows", cloud)
            checked += 1
    assert checked == 2 * 7


# ---------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------
def test_library_exports_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_sinkhorn_schedule", "pcm_sinkhorn_workspace_bytes", "pcm_sinkhorn_loss"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    for name, value in (("PCM_SINKHORN_MAX_POINTS", pcm_hip.SINKHORN_MAX_POINTS),
                        ("PCM_SINKHORN_MAX_STEPS", pcm_hip.SINKHORN_MAX_STEPS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == value
    assert (pcm_hip.SINKHORN_MAX_POINTS, pcm_hip.SINKHORN_MAX_STEPS) == (R.MAX_POINTS, R.MAX_STEPS) == (16384, 128)
    hip = open(os.path.join(CSRC, "sinkhorn.hip")).read()
    assert R.TILE == int(re.search(r"kSkTile\s*=\s*(\d+)", hip).group(1))
    assert R.WAVES == int(re.search(r"kSkWaves\s*=\s*(\d+)", hip).group(1))
    assert R.ROWS == 64 * int(re.search(r"kSkPerLane\s*=\s*(\d+)", hip).group(1))
    # geomloss is named as unverified wherever the formulas are stated
    assert "NOT verified" in src.split("Sinkhorn divergence (debiased")[1].split("EMD (auction")[0]
    assert "NOT verified" in hip and "NOT verified" in R.__doc__
    # no atomics, no waiting between workgroups, no __shfl chains
    lines = [ln.split("//", 1)[0] for ln in hip.splitlines()]
    assert not [ln for ln in lines if "atomic" in ln.lower() or "s_sleep" in ln or "__shfl" in ln]


def test_workspace_size():
    import pcm_hip
    need = pcm_hip.load_library().pcm_sinkhorn_workspace_bytes
    assert need(2, 300, 1025) == 2 * 2 * 1325 * 8  # two halves of two float32 potentials a point
    assert need(1, 1, 1) == 32 and need(32, 16384, 16384) == 2 * 32 * 32768 * 8
    assert need(0, 4, 4) == 0 and need(-1, 4, 4) == 0 and need(2, 0, 4) == 0 and need(2, 4, 0) == 0
    assert need(3, 300, 1025) > need(2, 300, 1025) and need(2, 301, 1025) > need(2, 300, 1025)


def _host_pointer():
    # a non-null, 8-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 8)
    addr = (ctypes.addressof(buf) + 7) & ~7
    return buf, ctypes.c_void_p(addr)


def test_sinkhorn_loss_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 40

    def call(b=2, n=8, m=9, l1=0, l2=0, blur=0.05, scaling=0.5, diameter=SQRT3, x=one, y=one, loss=one, g1=null,
             g2=null, pots=null, ws=one, ws_bytes=big):
        return lib.pcm_sinkhorn_loss(x, y, b, n, m, l1, l2, blur, scaling, diameter, loss, g1, g2, pots, ws,
                                     ws_bytes, null)

    assert call(b=-1) == INVALID and call(n=-8) == INVALID and call(m=-1) == INVALID
    assert call(l1=2) == INVALID and call(l2=-1) == INVALID
    for bad in (0.0, -0.2, NAN, INF, -INF):
        assert call(blur=bad) == INVALID and call(diameter=bad) == INVALID
    for bad in (0.0, 1.0, -0.5, 2.0, NAN, INF):
        assert call(scaling=bad) == INVALID
    assert call(blur=1e-3, scaling=0.99) == UNSUPPORTED  # too many steps
    assert call(b=0, blur=0.0) == INVALID and call(b=0, blur=1e-3, scaling=0.99) == UNSUPPORTED  # before b == 0
    assert call(n=-1, blur=1e-3, scaling=0.99) == INVALID  # sizes and layouts before the schedule
    # then b == 0 is a no-op, also with null pointers
    assert call(b=0) == OK
    assert call(b=0, n=0, m=0, x=null, y=null, loss=null, ws=null, ws_bytes=0) == OK
    assert call(n=0) == INVALID and call(m=0) == INVALID
    assert call(x=null) == INVALID and call(y=null) == INVALID and call(loss=null) == INVALID
    assert call(n=pcm_hip.SINKHORN_MAX_POINTS + 1) == UNSUPPORTED
    assert call(m=pcm_hip.SINKHORN_MAX_POINTS + 1) == UNSUPPORTED
    assert call(n=0, m=pcm_hip.SINKHORN_MAX_POINTS + 1) == INVALID  # invalid comes first
    assert call(n=pcm_hip.SINKHORN_MAX_POINTS, m=pcm_hip.SINKHORN_MAX_POINTS, ws=null) == WORKSPACE  # the limit is taken
    assert call(ws=null) == WORKSPACE
    assert call(ws_bytes=lib.pcm_sinkhorn_workspace_bytes(2, 8, 9) - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(one.value + 4)) == INVALID  # not 8-byte aligned
    del keep


def test_module_imports_without_a_device_and_raises():
    import kernel_loss
    import loss
    import sinkhorn_loss
    doc = " ".join(sinkhorn_loss.__doc__.split())
    assert "not verified" in doc and "sinkhorn_loop" in doc
    assert "capturable" in " ".join(sinkhorn_loss.SamplesLoss.__doc__.split())
    with pytest.raises(NotImplementedError, match="gaussian"):  # the kernel-norm module still does not offer it
        kernel_loss.SamplesLoss("sinkhorn")
    assert "sinkhorn_loss.py" in kernel_loss.__doc__
    L = sinkhorn_loss.SamplesLoss()
    assert (L.loss, L.p, L.blur, L.scaling, L.diameter) == ("sinkhorn", 2, 0.05, 0.5, None)
    for kwargs in ({"p": 1}, {"debias": False}, {"reach": 0.5}, {"potentials": True}, {"backend": "online"}):
        with pytest.raises(NotImplementedError):
            sinkhorn_loss.SamplesLoss("sinkhorn", **kwargs)
    with pytest.raises(NotImplementedError, match="sinkhorn"):
        sinkhorn_loss.SamplesLoss("hausdorff")
    for kwargs in ({"blur": 0.0}, {"scaling": 1.0}, {"scaling": 0.0}, {"diameter": -1.0}):
        with pytest.raises(ValueError):
            sinkhorn_loss.SamplesLoss("sinkhorn", **kwargs)
    # the kernel norms delegate
    K = sinkhorn_loss.SamplesLoss("gaussian", blur=0.2)
    assert isinstance(K.kernel, kernel_loss.SamplesLoss) and (K.kernel.loss, K.kernel.blur) == ("gaussian", 0.2)
    with pytest.raises(NotImplementedError):
        sinkhorn_loss.SamplesLoss("energy", reach=0.1)
    x, y = torch.rand(2, 10, 3), torch.rand(2, 12, 3)
    for M in (L, sinkhorn_loss.SamplesLoss("sinkhorn", diameter=2.0), K):
        with pytest.raises(RuntimeError):  # no CPU path
            M(x, y)
        with pytest.raises(RuntimeError):
            M(x[0], y[0])
        with pytest.raises(NotImplementedError):  # weighted clouds
            M(torch.ones(2, 10) / 10, x, torch.ones(2, 12) / 12, y)
    with pytest.raises(TypeError):
        L(x.double(), y.double())
    with pytest.raises(ValueError):
        L(x[:, :, :2], y)
    with pytest.raises(ValueError):
        L(x, y[:1])
    with pytest.raises(RuntimeError):
        loss.Loss().get_sinkhorn_loss(x, y)
    with pytest.raises(RuntimeError):
        loss.Loss().get_sinkhorn_loss(x.transpose(1, 2).contiguous().transpose(2, 1), y, diameter=2.0)
