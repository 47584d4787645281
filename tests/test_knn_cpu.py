"""k-nearest-neighbour and repulsion-loss checks that need no GPU: the library
exports and validates pcm_knn / pcm_repulsion_loss, the Python layers import
without a device and raise the documented errors, and the numpy restatement of
tests/knn_restated.py agrees with a float64 brute force where that is a fair
demand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import knn_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def test_library_exports_knn_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_knn", "pcm_repulsion_loss", "pcm_repulsion_workspace_bytes"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    assert pcm_hip.KNN_MAX_K == int(re.search(r"#define\s+PCM_KNN_MAX_K\s+(\d+)", src).group(1)) == 32
    assert pcm_hip.KNN_MAX_POINTS == int(re.search(r"#define\s+PCM_KNN_MAX_POINTS\s+(\d+)", src).group(1)) == 16384
    # the Python mirrors of the kernel's constants are the source's
    knn_src = open(os.path.join(CSRC, "knn.hip")).read()
    assert pcm_hip.KNN_TILE == int(re.search(r"kKnnTile\s*=\s*(\d+)", knn_src).group(1))
    assert pcm_hip.REPULSION_K == int(re.search(r"kRepK\s*=\s*(\d+)", knn_src).group(1)) == 5
    assert pcm_hip.REPULSION_POINTS == int(re.search(r"kRepPoints\s*=\s*(\d+)", knn_src).group(1))
    assert pcm_hip.KNN_WIDTHS[-1] == pcm_hip.KNN_MAX_K
    assert pcm_hip.KNN_SPLIT == int(re.search(r"kKnnSplit\s*=\s*(\d+)", knn_src).group(1))
    # small grids split the reference cloud over KNN_SPLIT waves, large ones do not
    below = int(re.search(r"kKnnSplitBelow\s*=\s*(\d+)", knn_src).group(1))
    assert pcm_hip.knn_default_split(32, 1024) == pcm_hip.KNN_SPLIT and pcm_hip.knn_default_split(8, 16384) == 1
    assert pcm_hip.knn_default_split(below - 1, 64) == pcm_hip.KNN_SPLIT and pcm_hip.knn_default_split(below, 64) == 1
    assert pcm_hip.knn_default_split(below - 1, 65) == 1
    # the workspace holds the k = 5 lists and a double per workgroup of points
    for b, n in ((1, 5), (2, 64), (3, 300), (8, 16384)):
        need = lib.pcm_repulsion_workspace_bytes(b, n)
        blocks = -(-n // pcm_hip.REPULSION_POINTS)
        assert need == 8 * b * blocks + 8 * 5 * b * n
    assert lib.pcm_repulsion_workspace_bytes(0, 64) == 0


def _host_pointer():
    # a non-null, 8-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 8)
    addr = (ctypes.addressof(buf) + 7) & ~7
    return buf, ctypes.c_void_p(addr)


@pytest.mark.parametrize("variant", [None, 0, 1, 2, 3])
def test_knn_rejects_bad_arguments_without_device(variant):
    import pcm_hip
    # the insert-at-once form lives in the tuning build; the product library refuses it
    lib = pcm_hip.load_tune_library() if variant == 1 else pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None

    def call(b=2, n=8, m=9, lq=0, lr=0, k=4, query=one, ref=one, dist=one, idx=one):
        if variant is None:
            return lib.pcm_knn(query, ref, b, n, m, lq, lr, k, dist, idx, null)
        return lib.pcm_tune_knn(variant, query, ref, b, n, m, lq, lr, k, dist, idx, null)

    # negative sizes, a layout outside {0, 1}, k < 1
    assert call(b=-1) == INVALID
    assert call(n=-8) == INVALID
    assert call(m=-1) == INVALID
    assert call(lq=2) == INVALID
    assert call(lr=-1) == INVALID
    assert call(k=0) == INVALID
    assert call(k=-3) == INVALID
    assert call(b=0, k=0) == INVALID  # before the b == 0 rule
    # then b == 0 is a no-op, also with null pointers
    assert call(b=0, query=null, ref=null, dist=null, idx=null) == OK
    assert call(b=0, n=0, m=0, query=null, ref=null, dist=null, idx=null) == OK
    # empty clouds or null pointers with b > 0
    assert call(n=0) == INVALID
    assert call(m=0) == INVALID
    assert call(query=null) == INVALID
    assert call(ref=null) == INVALID
    assert call(dist=null) == INVALID
    assert call(idx=null) == INVALID
    # above what the build supports
    assert call(k=pcm_hip.KNN_MAX_K + 1) == UNSUPPORTED
    assert call(n=pcm_hip.KNN_MAX_POINTS + 1) == UNSUPPORTED
    assert call(m=pcm_hip.KNN_MAX_POINTS + 1) == UNSUPPORTED
    del keep


def test_tune_knn_rejects_unknown_variant_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    assert lib.pcm_tune_knn(4, one, one, 2, 8, 8, 0, 0, 4, one, one, None) == INVALID
    assert lib.pcm_tune_knn(-1, one, one, 2, 8, 8, 0, 0, 4, one, one, None) == INVALID
    # valid arguments, but the form is not in the product library: refused before any device call
    assert lib.pcm_tune_knn(1, one, one, 2, 8, 8, 0, 0, 4, one, one, None) == UNSUPPORTED
    del keep


def test_repulsion_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 30

    def call(b=2, n=8, layout=0, h=0.01, xyz=one, loss=one, grad=null, ws=one, ws_bytes=big):
        return lib.pcm_repulsion_loss(xyz, b, n, layout, h, loss, grad, ws, ws_bytes, null)

    assert call(b=-1) == INVALID
    assert call(n=-8) == INVALID
    assert call(layout=2) == INVALID
    assert call(h=float("nan")) == INVALID
    assert call(h=float("inf")) == INVALID
    assert call(b=0, xyz=null, loss=null, ws=null, ws_bytes=0) == OK
    # fewer points than the list is long
    assert call(n=4) == INVALID
    assert call(n=0) == INVALID
    assert call(xyz=null) == INVALID
    assert call(loss=null) == INVALID
    assert call(n=pcm_hip.KNN_MAX_POINTS + 1) == UNSUPPORTED
    # a workspace that is missing or too short
    assert call(ws=null) == WORKSPACE
    assert call(ws_bytes=lib.pcm_repulsion_workspace_bytes(2, 8) - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(one.value + 4)) == INVALID  # not 8-byte aligned
    del keep


def test_modules_import_without_a_device_and_raise_on_bad_input():
    import knn
    import loss
    import repulsion_loss
    assert callable(knn.knn_points) and issubclass(knn.KNN, torch.nn.Module)
    assert "knn_cuda" in knn.__doc__ and "not installed" in knn.__doc__
    cloud = torch.rand(2, 16, 3)
    with pytest.raises(RuntimeError):
        knn.knn_points(cloud, cloud, 4)
    with pytest.raises(TypeError):
        knn.knn_points(cloud.double(), cloud.double(), 4)
    with pytest.raises(TypeError):
        knn.knn_points(cloud, cloud.half(), 4)
    with pytest.raises(ValueError):
        knn.knn_points(cloud[:, :, :2], cloud, 4)
    with pytest.raises(ValueError):
        knn.knn_points(cloud[0], cloud[0], 4)
    with pytest.raises(ValueError):
        knn.knn_points(cloud, cloud, 0)
    with pytest.raises(RuntimeError):
        knn.KNN(k=20, transpose_mode=True)(cloud, cloud)
    with pytest.raises(RuntimeError):
        knn.KNN(k=2)(cloud.transpose(1, 2), cloud.transpose(1, 2))
    with pytest.raises(ValueError):
        knn.KNN(k=2, transpose_mode=False)(cloud, cloud)  # [B, N, 3] where [B, 3, N] is due

    fn = repulsion_loss.repulsion_lossFunction.apply
    with pytest.raises(RuntimeError):
        fn(cloud, 0.01)
    with pytest.raises(RuntimeError):
        loss.Loss().get_repulsion_loss(cloud)
    with pytest.raises(TypeError):
        fn(cloud.double(), 0.01)
    with pytest.raises(ValueError):
        fn(cloud[:, :, :2], 0.01)
    with pytest.raises(ValueError):
        fn(cloud[:, :4], 0.01)


def test_restatement_agrees_with_float64_brute_force():
    rng = np.random.default_rng(5)
    b, n, m, k = 2, 24, 96, 8
    query = rng.random((b, n, 3), dtype=np.float32)
    ref = rng.random((b, m, 3), dtype=np.float32)
    d64 = ((ref.astype(np.float64)[:, None, :, :] - query.astype(np.float64)[:, :, None, :]) ** 2).sum(-1)
    # a fair demand only where no two candidates of a query are within 1e-6 relative
    s = np.sort(d64, axis=2)
    assert ((s[:, :, 1:] - s[:, :, :-1]) / s[:, :, 1:]).min() > 1e-6
    want = np.argsort(d64, axis=2)[:, :, :k]
    dist, idx = R.knn_restated(query, ref, k)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_allclose(dist, np.take_along_axis(d64, want, axis=2), rtol=1e-6)
    # rows= picks query rows
    rows = np.array([3, 17])
    sub_d, sub_i = R.knn_restated(query, ref, k, rows=rows)
    np.testing.assert_array_equal(sub_i, idx[:, rows])
    np.testing.assert_array_equal(sub_d, dist[:, rows])


def test_restatement_follows_the_slot_rules():
    cloud = np.array([[[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e19, 0, 0]]], np.float32)
    dist, idx = R.knn_restated(cloud, cloud, 4)
    # ties go to the lower index; NaN, +inf and overflowing candidates are never listed
    assert idx[0, 0].tolist() == [0, 1, 2, -1] and dist[0, 0].tolist() == [0.0, 1.0, 1.0, np.inf]
    assert idx[0, 2].tolist() == [1, 2, 0, -1]
    # a non-finite query lists nothing
    assert (idx[0, 3] == -1).all() and (idx[0, 4] == -1).all() and np.isinf(dist[0, 3]).all()
    # the far point lists itself only: every other distance overflows to +inf
    assert idx[0, 5].tolist() == [5, -1, -1, -1]
    # m < k leaves empty slots
    d2, i2 = R.knn_restated(cloud[:, :3], cloud[:, :2], 5)
    assert i2[0, 0].tolist() == [0, 1, -1, -1, -1] and np.isinf(d2[0, :, 2:]).all()
