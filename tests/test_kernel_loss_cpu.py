"""Kernel-norm loss checks that need no GPU: the numpy restatement of
tests/kernel_loss_restated.py agrees with torch float64 autograd and has the
properties of a kernel norm; the inputs of the GPU test are sensitive enough to
show a dropped tile or block; the library exports and validates
pcm_kernel_loss; loss/kernel_loss.py imports without a device and raises the
documented errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kernel_loss_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
NAN, INF = float("nan"), float("inf")


def _torch_loss(x, y, kernel, sigma):
    """The loss formula in torch float64, for autograd.  The square root's
    derivative is infinite at 0, so coincident pairs are masked out of r."""
    def k(p, q):
        d2 = ((p[:, None, :] - q[None, :, :]) ** 2).sum(-1)
        if kernel == R.GAUSSIAN:
            return torch.exp(-d2 / (2 * sigma * sigma))
        zero = d2 == 0
        r = torch.where(zero, torch.zeros_like(d2), torch.sqrt(torch.where(zero, torch.ones_like(d2), d2)))
        return torch.exp(-r / sigma) if kernel == R.LAPLACIAN else -r
    n, m = len(x), len(y)
    return 0.5 * k(x, x).sum() / (n * n) + 0.5 * k(y, y).sum() / (m * m) - k(x, y).sum() / (n * m)


@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_restated_gradients_equal_autograd(kernel):
    rng = np.random.default_rng(11)
    x, y = rng.random((5, 3), dtype=np.float32), rng.random((7, 3), dtype=np.float32)
    y[3] = y[1]  # a coincident pair inside a cloud
    y[6] = x[2]  # and one across the clouds
    for blur in (0.2, 1.0):
        sigma = float(np.float32(blur))
        L, gx, gy = R.restated_one(x, y, kernel, blur)
        tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        ty = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
        loss = _torch_loss(tx, ty, kernel, sigma)
        loss.backward()
        assert abs(loss.item() - L) <= 1e-14
        assert np.abs(tx.grad.numpy() - gx).max() <= 1e-13 and np.abs(ty.grad.numpy() - gy).max() <= 1e-13
        assert np.abs(gx).max() > 1e-3 and np.abs(gy).max() > 1e-3


@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_restated_is_a_kernel_norm(kernel):
    x, y = R.make_clouds(1, 40, 56)
    L, gx, gy = R.restated_one(x[0], x[0], kernel, 0.2)
    assert abs(L) <= 1e-15 and np.abs(gx).max() <= 1e-15 and np.abs(gy).max() <= 1e-15  # x = y
    L, _, _ = R.restated_one(x[0], y[0], kernel, 0.2)
    assert L > 1e-3  # distinct clouds
    # symmetric in the clouds, and unchanged by duplicating every point of one
    L2, hy, hx = R.restated_one(y[0], x[0], kernel, 0.2)
    assert abs(L2 - L) <= 1e-15
    L3, _, _ = R.restated_one(x[0], np.repeat(x[0], 2, axis=0), kernel, 0.2)
    assert abs(L3) <= 1e-15


def test_restated_at_the_reference_blur_is_the_diagonal():
    g = torch.Generator().manual_seed(5)
    x, y = torch.rand(64, 3, generator=g).numpy(), torch.rand(64, 3, generator=g).numpy()
    L, gx, gy = R.restated_one(x, y, R.GAUSSIAN, 5e-5)
    assert L == 0.5 * (1 / 64 + 1 / 64)
    assert (gx == 0).all() and (gy == 0).all()


def test_bounds_follow_the_library_constants():
    import pcm_hip
    assert (R.ROWS, R.TILE, R.WAVES) == (pcm_hip.KERNEL_LOSS_ROWS, pcm_hip.KERNEL_LOSS_TILE,
                                         pcm_hip.KERNEL_LOSS_WAVES)
    for n, m in [(1, 1), (255, 256), (257, 3), (1024, 1), (1025, 1024), (1300, 5), (16384, 2)]:
        assert R.chain(n, m) == pcm_hip.kernel_loss_chain(n, m)
    assert R.chain(1024, 1024) == 135 and R.chain(16384, 1) == 2055 and R.chain(1, 1) == 8
    assert R.chain(1025, 1) == 136 and R.chain(1300, 1) == 263
    assert R.EPS_EXP == 2.0 ** -21
    # the bounds grow with the chain and are what the derivation gives at one point
    assert R.loss_bound(R.GAUSSIAN, 1024, 1024) == pytest.approx(2 * (0.37 * 7 + 8 + 135 + 0.5) * 2.0 ** -24, rel=2e-3)
    assert R.grad_bound(R.ENERGY, 64, 32, 0.2)[1] == pytest.approx(2 * (3.5 + 2 + 71 + 3) * 2.0 ** -24 / 32, rel=2e-3)


@pytest.mark.parametrize("blur", R.BLURS)
@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_gpu_test_inputs_show_a_dropped_tile_or_block(kernel, blur):
    """A condition on the restatement and the inputs, not on any kernel: for
    every shape of the GPU test with n + m >= 128, leaving one tile of columns
    out of every row sum, or one block of rows out of the loss, moves the
    float64 loss by more than ten times the loss bound -- so the comparison
    within that bound would catch either.  The tile and the block are the
    first of each cloud: KERNEL_LOSS_TILE columns and KERNEL_LOSS_ROWS rows, or
    the whole cloud where it is shorter (its last, partial tile or block).  (A
    trailing tile or block of a single point is below the loss's resolution;
    the per-point gradient comparison covers those.)"""
    checked = 0
    for b, n, m in R.SHAPES:
        if n + m < 128:
            continue
        x, y = R.make_clouds(b, n, m)
        bound = R.loss_bound(kernel, n, m, R.diameter(x, y))
        for bi in range(b):
            mats = R.pair_matrices(x[bi], y[bi], kernel, blur)
            full = R.loss_from(mats)
            for cloud, c in ((0, n), (1, m)):
                cut = R.loss_from(mats, skip_cols=(cloud, 0, min(R.TILE, c)))
                assert abs(cut - full) > 10 * bound, (b, n, m, "columns", cloud, abs(cut - full) / bound)
                cut = R.loss_from(mats, skip_rows=(cloud, 0, min(R.ROWS, c)))
                assert abs(cut - full) > 10 * bound, (b, n, m, "rows", cloud, abs(cut - full) / bound)
                checked += 1
    assert checked >= 2 * 15


def test_library_exports_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_kernel_loss", "pcm_kernel_loss_workspace_bytes"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    for name, value in (("PCM_KERNEL_GAUSSIAN", pcm_hip.KERNEL_GAUSSIAN), ("PCM_KERNEL_LAPLACIAN", pcm_hip.KERNEL_LAPLACIAN),
                        ("PCM_KERNEL_ENERGY", pcm_hip.KERNEL_ENERGY),
                        ("PCM_KERNEL_LOSS_MAX_POINTS", pcm_hip.KERNEL_LOSS_MAX_POINTS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == value
    assert (pcm_hip.KERNEL_GAUSSIAN, pcm_hip.KERNEL_LAPLACIAN, pcm_hip.KERNEL_ENERGY) == R.KERNELS == (0, 1, 2)
    assert pcm_hip.KERNEL_LOSS_MAX_POINTS == 16384
    hip = open(os.path.join(CSRC, "kernel_loss.hip")).read()
    assert pcm_hip.KERNEL_LOSS_TILE == int(re.search(r"kKlTile\s*=\s*(\d+)", hip).group(1))
    assert pcm_hip.KERNEL_LOSS_WAVES == int(re.search(r"kKlWaves\s*=\s*(\d+)", hip).group(1))
    assert pcm_hip.KERNEL_LOSS_ROWS == 64 * int(re.search(r"kKlPerLane\s*=\s*(\d+)", hip).group(1))
    # geomloss is named as unverified wherever the formulas are stated
    assert "NOT verified" in src.split("Kernel-norm (MMD) losses")[1] and "NOT verified" in hip
    # no atomics, no waiting between workgroups, no __shfl chains
    lines = [ln.split("//", 1)[0] for ln in hip.splitlines()]
    assert not [ln for ln in lines if "atomic" in ln.lower() or "s_sleep" in ln or "__shfl" in ln]


def test_workspace_size():
    import pcm_hip
    lib = pcm_hip.load_library()
    need = lib.pcm_kernel_loss_workspace_bytes
    assert need(2, 300, 1025) == 2 * 1325 * 8  # two float32 sums a point
    assert need(1, 1, 1) > 0 and need(32, 16384, 16384) == 32 * 32768 * 8
    assert need(0, 4, 4) == 0 and need(-1, 4, 4) == 0 and need(2, 0, 4) == 0 and need(2, 4, 0) == 0
    assert need(3, 300, 1025) > need(2, 300, 1025) and need(2, 301, 1025) > need(2, 300, 1025)


def _host_pointer():
    # a non-null, 8-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 8)
    addr = (ctypes.addressof(buf) + 7) & ~7
    return buf, ctypes.c_void_p(addr)


def test_kernel_loss_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 40

    def call(b=2, n=8, m=9, l1=0, l2=0, kernel=0, blur=0.2, x=one, y=one, loss=one, g1=null, g2=null, ws=one,
             ws_bytes=big):
        return lib.pcm_kernel_loss(x, y, b, n, m, l1, l2, kernel, blur, loss, g1, g2, ws, ws_bytes, null)

    assert call(b=-1) == INVALID and call(n=-8) == INVALID and call(m=-1) == INVALID
    assert call(l1=2) == INVALID and call(l2=-1) == INVALID
    assert call(kernel=-1) == INVALID and call(kernel=3) == INVALID
    for bad in (0.0, -0.2, NAN, INF, -INF):
        for kernel in R.KERNELS:  # for the energy distance too, which does not use it
            assert call(blur=bad, kernel=kernel) == INVALID
    assert call(b=0, kernel=3) == INVALID and call(b=0, blur=0.0) == INVALID  # before the b == 0 rule
    # then b == 0 is a no-op, also with null pointers
    assert call(b=0) == OK
    assert call(b=0, n=0, m=0, x=null, y=null, loss=null, ws=null, ws_bytes=0) == OK
    assert call(n=0) == INVALID and call(m=0) == INVALID
    assert call(x=null) == INVALID and call(y=null) == INVALID and call(loss=null) == INVALID
    assert call(n=pcm_hip.KERNEL_LOSS_MAX_POINTS + 1) == UNSUPPORTED
    assert call(m=pcm_hip.KERNEL_LOSS_MAX_POINTS + 1) == UNSUPPORTED
    assert call(n=0, m=pcm_hip.KERNEL_LOSS_MAX_POINTS + 1) == INVALID  # invalid comes first
    assert call(n=pcm_hip.KERNEL_LOSS_MAX_POINTS, m=pcm_hip.KERNEL_LOSS_MAX_POINTS, ws=null) == WORKSPACE  # the limit is taken
    assert call(ws=null) == WORKSPACE
    assert call(ws_bytes=lib.pcm_kernel_loss_workspace_bytes(2, 8, 9) - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(one.value + 4)) == INVALID  # not 8-byte aligned
    for kernel in R.KERNELS:
        assert call(kernel=kernel, ws=null) == WORKSPACE  # every kernel is accepted
    del keep


def test_module_imports_without_a_device_and_raises():
    import kernel_loss
    import loss_
    doc = " ".join(kernel_loss.__doc__.split())
    assert "not verified" in doc and "1e-8" in doc and "trains nothing" in doc
    assert "kernel_loss" in loss_.__doc__ and not hasattr(loss_, "batch_EMD_loss")
    for name in ("sinkhorn", "hausdorff", "emd"):
        with pytest.raises(NotImplementedError, match="gaussian"):
            kernel_loss.SamplesLoss(name)
    with pytest.raises(NotImplementedError):
        kernel_loss.SamplesLoss("gaussian", reach=0.1)
    with pytest.raises(ValueError):
        kernel_loss.SamplesLoss("gaussian", blur=0.0)
    x, y = torch.rand(2, 10, 3), torch.rand(2, 12, 3)
    for name in ("gaussian", "laplacian", "energy"):
        L = kernel_loss.SamplesLoss(name, blur=0.2)
        with pytest.raises(RuntimeError):  # no CPU path
            L(x, y)
        with pytest.raises(RuntimeError):
            L(x[0], y[0])
        with pytest.raises(NotImplementedError):  # weighted clouds
            L(torch.ones(2, 10) / 10, x, torch.ones(2, 12) / 12, y)
    L = kernel_loss.SamplesLoss()
    assert (L.loss, L.p, L.blur) == ("gaussian", 2, 0.05)
    with pytest.raises(TypeError):
        L(x.double(), y.double())
    with pytest.raises(ValueError):
        L(x[:, :, :2], y)
    with pytest.raises(ValueError):
        L(x, y[:1])
    with pytest.raises(RuntimeError):
        kernel_loss.batch_EMD_loss(x, y)
