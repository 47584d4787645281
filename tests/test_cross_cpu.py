"""Cross Chamfer matrix checks that need no GPU: the library's exports,
constants, validation and workspace size through the C-ABI; cross_chamfer_3D's
argument handling without a device; utils/set_metrics.py on hand-built matrices
against the loops of tests/cross_restated.py; and the tolerance's own check --
that float64 sums in any fixed order stay within the 1-ulp / 0.1 % rule the GPU
test holds the kernel to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cross_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


# ---------------------------------------------------------------------------
# the library
# ---------------------------------------------------------------------------
def test_library_exports_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_chamfer_cross_workspace_bytes", "pcm_chamfer_cross"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    assert int(re.search(r"#define\s+PCM_CROSS_MAX_POINTS\s+(\d+)", src).group(1)) == pcm_hip.CROSS_MAX_POINTS == 16384
    assert (pcm_hip.CROSS_QUERIES, pcm_hip.CROSS_TILE, pcm_hip.CROSS_J, pcm_hip.CROSS_MIN_BLOCKS) == (
        R.QUERIES, R.TILE, R.J, R.MIN_BLOCKS)
    hip = open(os.path.join(CSRC, "chamfer_cross.hip")).read()
    for const, value in (("kCrossW", 4), ("kCrossQPT", 4), ("kCrossTile", R.TILE), ("kCrossJ", R.J),
                         ("kCrossWantBlocks", R.MIN_BLOCKS)):
        assert re.search(r"constexpr\s+(int|long long)\s+" + const + r"\s*=\s*" + str(value) + r"\s*;", hip), const
    assert 64 * 4 * 4 == R.QUERIES
    # the rules tests/test_build_cpu.py holds the older hot files to; no atomics, no waiting between workgroups
    lines = [ln.split("//", 1)[0] for ln in hip.splitlines()]
    assert not [ln for ln in lines if "__syncthreads_or" in ln or "__syncthreads_and" in ln or "__syncthreads_count" in ln]
    assert not [ln for ln in lines if "__shfl" in ln]
    assert not [ln for ln in lines if "atomic" in ln.lower() or "s_sleep" in ln]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "-ffp-contract=off" in makefile and makefile.count("chamfer_cross") == 2  # NAMES and the tuning build


def test_run_lengths_of_the_edge_shapes():
    import pcm_hip
    for shape, run in R.EDGE_RUNS.items():
        assert pcm_hip.chamfer_cross_run(*shape) == run, shape
    assert pcm_hip.chamfer_cross_run(0, 4, 4, 4) == 0
    assert pcm_hip.chamfer_cross_run(32, 1024, 1024, 1024) == R.J  # the retrieval shape streams full runs
    for shape in R.SHAPES:  # a run is a power of two no longer than J, and 1 leaves nothing to halve
        assert pcm_hip.chamfer_cross_run(*shape) in (1, 2, 4, 8)


def test_workspace_size():
    import pcm_hip
    need = pcm_hip.load_library().pcm_chamfer_cross_workspace_bytes
    for args in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, -4, 4, 4), (0, 0, 0, 0)):
        assert need(*args) == 0, args
    assert need(1, 1, 1, 1) > 0 and need(1, 1, 1, 1) % 128 == 0
    # one float64 record per entry, direction and query block
    assert need(3, 5, 1024, 1024) >= 3 * 5 * 2 * 8
    assert need(3, 5, 2049, 1024) >= 3 * 5 * (3 + 1) * 8
    assert need(64, 32, 1024, 1024) > need(32, 32, 1024, 1024) > need(32, 16, 1024, 1024)  # grows with s and r
    assert need(32, 32, 4096, 1024) > need(32, 32, 2048, 1024) > need(32, 32, 1024, 1024)  # and with n
    assert need(32, 32, 1024, 16384) > need(32, 32, 1024, 1024)
    assert need(1 << 16, 1 << 16, 4, 4) == 0  # s r beyond the launch limits: the call is unsupported
    assert pcm_hip.chamfer_cross_workspace_bytes(3, 5, 2049, 1024) == need(3, 5, 2049, 1024)


def _host_pointer():
    # a non-null, 16-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 16)
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_chamfer_cross_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 44
    over = pcm_hip.CROSS_MAX_POINTS + 1

    def call(s=2, r=3, n=8, m=9, l1=0, l2=0, x=one, y=one, m12=one, m21=one, ws=one, ws_bytes=big):
        return lib.pcm_chamfer_cross(x, y, s, r, n, m, l1, l2, m12, m21, ws, ws_bytes, null)

    assert call(s=-1) == INVALID and call(r=-1) == INVALID and call(n=-8) == INVALID and call(m=-1) == INVALID
    assert call(l1=2) == INVALID and call(l2=-1) == INVALID and call(l1=-1, l2=5) == INVALID
    assert call(s=0, l1=3) == INVALID and call(r=0, n=-1) == INVALID  # before the empty problem
    # an empty set is a no-op, also with null pointers and no workspace
    assert call(s=0) == OK and call(r=0) == OK
    assert call(s=0, r=0, n=0, m=0, x=null, y=null, m12=null, m21=null, ws=null, ws_bytes=0) == OK
    assert call(s=0, n=over) == OK
    assert call(n=0) == INVALID and call(m=0) == INVALID
    assert call(x=null) == INVALID and call(y=null) == INVALID and call(m12=null) == INVALID
    assert call(n=over) == UNSUPPORTED and call(m=over) == UNSUPPORTED
    assert call(s=1 << 16, r=1 << 16) == UNSUPPORTED  # s r beyond the launch limits
    assert call(s=1 << 15, r=1 << 15, n=over - 1, m=4) == UNSUPPORTED  # the grid beyond them: 2^31 workgroups
    assert call(n=0, m=over) == INVALID and call(x=null, n=over) == INVALID  # invalid comes first
    # the limits themselves are taken; mean21 is optional
    assert call(n=pcm_hip.CROSS_MAX_POINTS, m=pcm_hip.CROSS_MAX_POINTS, ws=null) == WORKSPACE
    assert call(ws=null) == WORKSPACE and call(m21=null, ws=null) == WORKSPACE and call(ws=null, ws_bytes=0) == WORKSPACE
    assert call(ws_bytes=lib.pcm_chamfer_cross_workspace_bytes(2, 3, 8, 9) - 1) == WORKSPACE
    assert call(n=2049, ws_bytes=lib.pcm_chamfer_cross_workspace_bytes(2, 3, 1024, 9)) == WORKSPACE
    assert call(n=over, ws=null) == UNSUPPORTED  # before the workspace
    assert call(ws=ctypes.c_void_p(one.value + 4)) == INVALID  # not 8-byte aligned
    del keep


# ---------------------------------------------------------------------------
# the Python layer without a device
# ---------------------------------------------------------------------------
def test_module_imports_without_a_device_and_raises():
    import cross_chamfer_3D as C
    import pcm_hip
    import set_metrics
    x, y = torch.rand(2, 10, 3), torch.rand(3, 12, 3)
    for fn in (C.chamfer_cross, C.chamfer_3DCross()):
        with pytest.raises(RuntimeError):  # no CPU path
            fn(x, y)
        with pytest.raises(RuntimeError):
            fn(x)
        with pytest.raises(TypeError):
            fn(x.double(), y.double())
        with pytest.raises(TypeError):
            fn(x.half())
        with pytest.raises(TypeError):
            fn(x.double(), y)
        with pytest.raises(ValueError):
            fn(x[0], y)  # wrong rank
        with pytest.raises(ValueError):
            fn(x, y[:, :, :2])  # last dimension
        with pytest.raises(ValueError):
            fn(x.reshape(2, 10, 3, 1))
    with pytest.raises(RuntimeError):  # the binding itself
        pcm_hip.chamfer_cross(x, 0, y, 0, torch.empty(2, 3))
    with pytest.raises(RuntimeError):
        set_metrics.nearest_shape(x, y)
    with pytest.raises(RuntimeError):
        set_metrics.compute_set_metrics(x, y)
    assert C.ChamferCross._fields == ("mean12", "mean21", "cd")
    doc = " ".join(set_metrics.__doc__.split())
    assert "stated from the publications, not verified against their packages" in doc


# ---------------------------------------------------------------------------
# the set metrics on hand-built matrices
# ---------------------------------------------------------------------------
def _check_metrics(cd_sr, cd_ss=None, cd_rr=None):
    import set_metrics
    cd_sr = np.asarray(cd_sr, dtype=np.float32)
    t = torch.from_numpy(cd_sr)
    val, idx = torch.min(t, dim=1)  # what set_metrics.nearest_shape applies to the matrix
    want_idx, want_val = R.nearest_shape(cd_sr)
    assert np.array_equal(idx.numpy(), want_idx) and np.array_equal(val.numpy(), want_val)
    mmd, cov = set_metrics.mmd_cov(t)
    want_mmd, want_cov = R.mmd_cov(cd_sr)
    assert abs(mmd - want_mmd) <= 1e-12 * max(abs(want_mmd), 1e-30) and cov == want_cov
    acc = None
    if cd_ss is not None:
        cd_ss, cd_rr = np.asarray(cd_ss, dtype=np.float32), np.asarray(cd_rr, dtype=np.float32)
        acc = set_metrics.one_nna(torch.from_numpy(cd_ss), t, torch.from_numpy(cd_rr))
        assert acc == R.one_nna(cd_ss, cd_sr, cd_rr)
    return mmd, cov, acc


def test_set_metrics_ties_go_to_the_lowest_index():
    cd = [[2, 1, 1, 3], [5, 5, 5, 5], [0, 7, 0, 7]]  # S = 3, R = 4: every row and two columns tie
    mmd, cov, _ = _check_metrics(cd)
    assert cov == 2 / 4  # rows choose references 1, 0, 0
    assert mmd == (0 + 1 + 0 + 3) / 4
    want_idx, _ = R.nearest_shape(np.asarray(cd, dtype=np.float32))
    assert list(want_idx) == [1, 0, 0]


def test_set_metrics_rectangular_and_unselected_reference():
    rng = np.random.default_rng(5)
    cd = rng.random((5, 7), dtype=np.float32)  # S < R: at most 5 of 7 references can be covered
    mmd, cov, _ = _check_metrics(cd)
    assert cov <= 5 / 7 < 1
    cd = rng.random((9, 4), dtype=np.float32)
    cd[:, 2] += 10  # no sample selects reference 2
    mmd, cov, _ = _check_metrics(cd)
    assert cov <= 3 / 4
    assert mmd > 2.0  # its column's minimum is in the mean


def test_set_metrics_single_sample_and_single_reference():
    mmd, cov, acc = _check_metrics([[3.0, 1.0, 2.0]], [[0.0]], np.ones((3, 3)) - np.eye(3))
    assert (mmd, cov) == (2.0, 1 / 3)
    mmd, cov, acc = _check_metrics([[3.0], [1.0], [2.0]], np.ones((3, 3)) - np.eye(3), [[0.0]])
    assert (mmd, cov) == (1.0, 1.0)
    mmd, cov, acc = _check_metrics([[4.0]], [[0.0]], [[0.0]])
    assert (mmd, cov, acc) == (4.0, 1.0, 0.0)  # each cloud's only neighbour is of the other set


def test_one_nna_on_separated_and_identical_sets():
    import set_metrics
    s, r = 4, 6
    near_s, near_r = np.full((s, s), 0.1, np.float32), np.full((r, r), 0.2, np.float32)
    np.fill_diagonal(near_s, 0)
    np.fill_diagonal(near_r, 0)
    far = np.full((s, r), 9.0, np.float32)
    assert _check_metrics(far, near_s, near_r)[2] == 1.0  # perfectly separated blocks
    # identical sets: cloud a's nearest other cloud is its own copy in the other set (distance 0)
    rng = np.random.default_rng(6)
    own = rng.random((5, 5)).astype(np.float32) + 1
    own = own + own.T
    np.fill_diagonal(own, 0)
    assert _check_metrics(own, own, own)[2] == 0.0
    # the diagonal is excluded whatever it holds
    t = torch.from_numpy(own)
    assert set_metrics.one_nna(t - 5 * torch.eye(5), t, t) == 0.0
    with pytest.raises(ValueError):
        set_metrics.one_nna(t, t[:, :3], t)
    with pytest.raises(ValueError):
        set_metrics.mmd_cov(torch.zeros(0, 3))


# ---------------------------------------------------------------------------
# the tolerance's own check
# ---------------------------------------------------------------------------
def _orders(d):
    """float32(sum / n) of the rows of d [k, n] in three fixed float64 orders."""
    n = d.shape[-1]
    d64 = d.astype(np.float64)
    fwd, rev = np.zeros(len(d64)), np.zeros(len(d64))
    for k in range(n):
        fwd += d64[:, k]
        rev += d64[:, n - 1 - k]
    parts = np.zeros((8, len(d64)))
    for p in range(8):  # eight strided partials, each ascending, merged ascending
        for k in range(p, n, 8):
            parts[p] += d64[:, k]
    merged = np.zeros(len(d64))
    for p in range(8):
        merged += parts[p]
    return [(v / n).astype(np.float32) for v in (fwd, rev, merged)]


def test_any_fixed_float64_order_is_within_the_rule():
    tally = R.Tally()
    for shape in R.SMALL_SHAPES:
        x, y = R.make_sets(*shape)
        d1, d2 = R.pair_distances(x, y)
        for d in (d1, d2):
            rows = d.reshape(-1, d.shape[-1])
            want = R.mean_exact(rows)
            for k, got in enumerate(_orders(rows)):
                tally.check(got, want, f"{R.shape_id(shape)} order {k}")
    assert tally.entries > 10000
    print(f"{tally.inexact} of {tally.entries} entries not bit-equal")
    assert tally.share() <= R.MAX_INEXACT_SHARE


def test_restatement_matches_a_brute_force_double_loop():
    x, y = R.make_sets(2, 3, 6, 5)
    m12, m21 = R.cross_means(x, y)
    for i in range(2):
        for j in range(3):
            dd = ((x[i][:, None, :].astype(np.float64) - y[j][None, :, :]) ** 2).sum(axis=2)
            assert abs(m12[i, j] - dd.min(axis=1).mean()) <= 1e-6
            assert abs(m21[i, j] - dd.min(axis=0).mean()) <= 1e-6
    assert not np.allclose(m12, m21)
