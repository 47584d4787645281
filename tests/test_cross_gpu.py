"""The cross Chamfer matrix on the GPU (pcm_chamfer_cross, csrc/chamfer_cross.hip)
against the restatement of tests/cross_restated.py: np.float32(fsum(d) / n) of the
oracle's per-point distances.  The rule, everywhere: an entry is at most 1 ulp
off, and at most 0.1 % of all entries compared in this file are not bit-equal
(the last test); tests/test_cross_cpu.py shows that float64 sums in any fixed
order meet it.  Every output is prefilled with a sentinel that the call must
overwrite."""
import numpy as np
import pytest
import torch

import cross_restated as R
import geometry_cases as G

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
TALLY = R.Tally()


def _dev(cuda, a, planes=False):
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(cuda)  # a copy: the references are read-only
    if planes:  # a [S, N, 3] view of contiguous channel planes [S, 3, N]
        t = t.transpose(1, 2).contiguous().transpose(1, 2)
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _cross(cuda, x, y, planes=(False, False), both=True, workspace=None):
    """(mean12, mean21 or None) as numpy from the binding, sentinels checked."""
    import pcm_hip
    xt = x if isinstance(x, torch.Tensor) else _dev(cuda, x, planes[0])
    yt = y if isinstance(y, torch.Tensor) else _dev(cuda, y, planes[1])
    s, r = xt.shape[0], yt.shape[0]
    m12 = torch.full((s, r), SENTINEL, device=cuda)
    m21 = torch.full((s, r), SENTINEL, device=cuda) if both else None
    pcm_hip.chamfer_cross(xt, pcm_hip.cloud_layout(xt), yt, pcm_hip.cloud_layout(yt), m12, m21, workspace=workspace)
    torch.cuda.synchronize()
    outs = [t.cpu().numpy() if t is not None else None for t in (m12, m21)]
    for o in outs:
        assert o is None or not (o == SENTINEL).any(), "an entry was not written"
    return outs


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_values_match_the_restatement(cuda, shape):
    x, y, want12, want21 = R.reference(shape)
    got12, got21 = _cross(cuda, x, y)
    TALLY.check(got12, want12, f"{R.shape_id(shape)} mean12")
    TALLY.check(got21, want21, f"{R.shape_id(shape)} mean21")
    if shape[0] * shape[1] > 1 and shape[2] != shape[3]:
        assert not np.array_equal(got12, got21)  # a transposed or swapped mean21 would not pass above


@pytest.mark.parametrize("shape", [(2, 3, 64, 65), (2, 2, 1030, 300)], ids=R.shape_id)
def test_values_match_the_products_own_forward(cuda, shape):
    import dist_chamfer_3D
    x, y = R.make_sets(*shape, seed=77)
    xt, yt = _dev(cuda, x), _dev(cuda, y)
    got12, got21 = _cross(cuda, xt, yt)
    want12, want21 = np.empty_like(got12), np.empty_like(got21)
    fwd = dist_chamfer_3D.chamfer_3DDist()
    for i in range(shape[0]):
        for j in range(shape[1]):
            d1, d2, _, _ = fwd(xt[i:i + 1], yt[j:j + 1])
            want12[i, j] = R.mean_exact(d1.cpu().numpy())[0]
            want21[i, j] = R.mean_exact(d2.cpu().numpy())[0]
    TALLY.check(got12, want12, f"{R.shape_id(shape)} mean12 against chamfer_3DDist")
    TALLY.check(got21, want21, f"{R.shape_id(shape)} mean21 against chamfer_3DDist")


# ---------------------------------------------------------------------------
# bit-identity
# ---------------------------------------------------------------------------
IDENT_SHAPE = (5, 9, 1030, 300)  # two query blocks in direction 1, one in direction 2; r = J + 1


def test_runs_layouts_and_the_optional_output_agree_bit_for_bit(cuda):
    x, y = R.make_sets(*IDENT_SHAPE, seed=31)
    base12, base21 = _cross(cuda, x, y)
    again12, again21 = _cross(cuda, x, y)
    assert np.array_equal(_bits(base12), _bits(again12)) and np.array_equal(_bits(base21), _bits(again21))
    for planes in ((True, False), (False, True), (True, True)):
        p12, p21 = _cross(cuda, x, y, planes=planes)
        assert np.array_equal(_bits(base12), _bits(p12)) and np.array_equal(_bits(base21), _bits(p21)), planes
    only12, none = _cross(cuda, x, y, both=False)
    assert none is None and np.array_equal(_bits(base12), _bits(only12))
    only12, _ = _cross(cuda, x, y, planes=(True, True), both=False)
    assert np.array_equal(_bits(base12), _bits(only12))


def test_an_entry_equals_the_one_by_one_call(cuda):
    x, y = R.make_sets(*IDENT_SHAPE, seed=31)
    xt, yt = _dev(cuda, x), _dev(cuda, y)
    base12, base21 = _cross(cuda, xt, yt)
    for i in range(IDENT_SHAPE[0]):
        for j in range(IDENT_SHAPE[1]):
            one12, one21 = _cross(cuda, xt[i:i + 1], yt[j:j + 1])
            assert _bits(one12)[0, 0] == _bits(base12)[i, j] and _bits(one21)[0, 0] == _bits(base21)[i, j], (i, j)


def test_equal_gallery_clouds_give_equal_columns_and_a_permutation_permutes(cuda):
    x, y = R.make_sets(*IDENT_SHAPE, seed=31)
    y = y.copy()
    y[6] = y[3]
    base12, base21 = _cross(cuda, x, y)
    assert np.array_equal(_bits(base12[:, 3]), _bits(base12[:, 6]))
    assert np.array_equal(_bits(base21[:, 3]), _bits(base21[:, 6]))
    assert not np.array_equal(base12[:, 3], base12[:, 4])
    perm = np.random.default_rng(3).permutation(IDENT_SHAPE[1])
    assert not np.array_equal(perm, np.arange(IDENT_SHAPE[1]))
    p12, p21 = _cross(cuda, x, y[perm])
    assert np.array_equal(_bits(p12), _bits(base12[:, perm])) and np.array_equal(_bits(p21), _bits(base21[:, perm]))
    rows = perm[:IDENT_SHAPE[0]] % IDENT_SHAPE[0]
    q12, q21 = _cross(cuda, x[rows], y)
    assert np.array_equal(_bits(q12), _bits(base12[rows])) and np.array_equal(_bits(q21), _bits(base21[rows]))


# ---------------------------------------------------------------------------
# the Python API: self mode
# ---------------------------------------------------------------------------
def test_self_mode_is_symmetric_with_a_zero_diagonal_and_equals_the_pair_call(cuda):
    import cross_chamfer_3D as C
    x, _ = R.make_sets(6, 1, 1030, 1, seed=41)
    for planes in (False, True):
        xt = _dev(cuda, x, planes).requires_grad_(True)
        own = C.chamfer_cross(xt)
        pair = C.chamfer_3DCross()(xt, xt)
        torch.cuda.synchronize()
        for t in own + pair:
            assert tuple(t.shape) == (6, 6) and t.dtype == torch.float32 and not t.requires_grad
        assert torch.equal(own.cd, own.cd.t())
        assert torch.equal(torch.diagonal(own.cd), torch.zeros(6, device=cuda))
        assert torch.equal(torch.diagonal(own.mean12), torch.zeros(6, device=cuda))
        for a, b in zip(own, pair):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
        assert torch.equal(own.mean21, own.mean12.t()) and torch.equal(own.cd, own.mean12 + own.mean21)
        assert float(own.cd.sum()) > 0
    # other strides are made contiguous: every second point of a larger set
    wide = _dev(cuda, R.make_sets(3, 1, 80, 1, seed=42)[0])
    sliced = C.chamfer_cross(wide[:, ::2], wide)
    dense = C.chamfer_cross(wide[:, ::2].contiguous(), wide)
    for a, b in zip(sliced, dense):
        assert torch.equal(a, b)
    empty = C.chamfer_cross(wide[:0], wide)
    assert tuple(empty.cd.shape) == (0, 3)


# ---------------------------------------------------------------------------
# geometry (tests/geometry_cases.py, at the F-score op's first shape)
# ---------------------------------------------------------------------------
GEOMETRY = ("scale_1e3", "scale_1e-20", "offset_1000", "collapsed", "identical", "far_point")


@pytest.mark.parametrize("family", GEOMETRY)
def test_geometry_families(cuda, family):
    c = G.case("fscore", family, G.SHAPES["fscore"][0])  # x [2, 300, 3], y [2, 1025, 3] ([2, 300, 3] for identical)
    want12, want21 = R.cross_means(c.x, c.y)
    got12, got21 = _cross(cuda, c.x, c.y)
    TALLY.check(got12, want12, f"{family} mean12")
    TALLY.check(got21, want21, f"{family} mean21")
    if family == "scale_1e-20":  # every distance is a float32 subnormal; the float64 sum keeps them
        assert (want12 > 0).all() and (want12 < 1e-38).all() and (got12 > 0).all() and (got21 > 0).all()
    if family == "identical":
        assert not np.diagonal(got12).any() and not np.diagonal(got21).any() and got12[0, 1] > 0
    if family == "far_point":
        assert (got21 > 1.0).all()  # the outlier's 30^2-scale distance is in every mean over y


# ---------------------------------------------------------------------------
# non-finite input, errors, capture
# ---------------------------------------------------------------------------
def test_non_finite_clouds_touch_only_their_row_and_column(cuda):
    x, y = R.make_sets(4, 10, 300, 1030, seed=51)
    x, y = x.copy(), y.copy()
    clean12, clean21 = _cross(cuda, x, y)
    bad_x, bad_y = x.copy(), y.copy()
    bad_x[2, 7, 1] = np.nan
    bad_x[2, 290, 0] = np.inf
    bad_y[5, 1029, 2] = np.nan
    bad_y[5, 3, 0] = -np.inf
    got12, got21 = _cross(cuda, bad_x, bad_y)  # returns, and every entry is written (_cross checks the sentinel)
    keep = np.ones((4, 10), dtype=bool)
    keep[2, :] = False
    keep[:, 5] = False
    assert np.array_equal(_bits(got12)[keep], _bits(clean12)[keep])
    assert np.array_equal(_bits(got21)[keep], _bits(clean21)[keep])


def test_short_workspace_raises(cuda):
    import pcm_hip
    x, y = R.make_sets(2, 3, 64, 65)
    need = pcm_hip.chamfer_cross_workspace_bytes(2, 3, 64, 65)
    with pytest.raises(pcm_hip.PcmError):
        _cross(cuda, x, y, workspace=torch.empty(need - 1, dtype=torch.uint8, device=cuda))
    exact = torch.full((need,), 255, dtype=torch.uint8, device=cuda)  # needs no initialisation
    got12, got21 = _cross(cuda, x, y, workspace=exact)
    ref = R.reference((2, 3, 64, 65))
    TALLY.check(got12, ref[2], "exact workspace mean12")
    TALLY.check(got21, ref[3], "exact workspace mean21")
    with pytest.raises(pcm_hip.PcmError):
        _cross(cuda, np.zeros((1, pcm_hip.CROSS_MAX_POINTS + 1, 3), np.float32), y)


def test_graph_capture_replays_bit_identically(cuda):
    import cross_chamfer_3D as C
    shape = (3, 9, 1030, 300)  # scan and finalise launches
    first, second = R.make_sets(*shape, seed=61), R.make_sets(*shape, seed=62)
    eager = []
    for x, y in (first, second):
        res = C.chamfer_cross(_dev(cuda, x), _dev(cuda, y))
        eager.append([t.cpu().numpy() for t in res])
    sx, sy = _dev(cuda, first[0]), _dev(cuda, first[1])
    out = {}

    def call():
        out["res"] = C.chamfer_cross(sx, sy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for replay, (clouds, want) in enumerate(((second, eager[1]), (first, eager[0]))):
        sx.copy_(_dev(cuda, clouds[0]))
        sy.copy_(_dev(cuda, clouds[1]))
        for t in out["res"]:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        for t, w in zip(out["res"], want):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(w)), replay


# ---------------------------------------------------------------------------
# the set metrics on the GPU's own matrices
# ---------------------------------------------------------------------------
def test_set_metrics_equal_the_restatement_fed_the_gpu_matrices(cuda):
    import cross_chamfer_3D as C
    import set_metrics
    sample, ref = R.make_sets(5, 7, 64, 64, seed=71)
    ref = ref.copy()
    ref[4] = sample[2]  # an exact duplicate across the sets: distance 0
    st, rt = _dev(cuda, sample), _dev(cuda, ref)
    cd_sr = C.chamfer_cross(st, rt).cd.cpu().numpy()
    cd_ss = C.chamfer_cross(st).cd.cpu().numpy()
    cd_rr = C.chamfer_cross(rt).cd.cpu().numpy()
    idx, val = set_metrics.nearest_shape(st, rt)
    want_idx, want_val = R.nearest_shape(cd_sr)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(want_val))
    assert want_idx[2] == 4 and want_val[2] == 0
    got = set_metrics.compute_set_metrics(st, rt)
    mmd, cov = R.mmd_cov(cd_sr)
    assert sorted(got) == ["1-NNA-CD", "COV-CD", "MMD-CD"]
    assert abs(got["MMD-CD"] - mmd) <= 1e-12 * mmd and got["COV-CD"] == cov
    assert got["1-NNA-CD"] == R.one_nna(cd_ss, cd_sr, cd_rr)
    assert 0 < got["COV-CD"] <= 5 / 7 and 0 <= got["1-NNA-CD"] <= 1


def test_share_of_entries_not_bit_equal(cuda):
    """Last in the file: over everything compared above."""
    print(f"{TALLY.inexact} of {TALLY.entries} entries not bit-equal")
    assert TALLY.entries > 10000
    assert TALLY.share() <= R.MAX_INEXACT_SHARE
