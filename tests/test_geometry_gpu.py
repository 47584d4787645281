"""The newer losses' HIP kernels on tests/geometry_cases.py -- clouds outside
the unit cube and on degenerate geometry -- against the numpy restatements of
their contracts: pcm_knn, pcm_fps, pcm_ball_query and the uniform loss's
groups EQUAL to the restatement; pcm_repulsion_loss, pcm_uniform_loss,
pcm_kernel_loss, pcm_sinkhorn_loss, pcm_sliced_wasserstein_loss and
pcm_dcd_loss within the modules' own derived bounds evaluated on the case
(Sinkhorn: the tolerances of geometry_cases.sinkhorn_reference, which
tests/test_geometry_cpu.py holds between its two conditions); and the ninth
op, pcm_chamfer_eval (the one-pass evaluation behind fscore): counts EQUAL to
the oracle's distances counted under the thresholds, scores the pinned float32
arithmetic on them bit for bit, mean distances within rtol 1e-5.  Every case is
run twice through the cached workspace with a call of another family (1e3-scale
data) in between and must give the same bits; `generator` is repeated with x
as a planes view.

Every case prints its largest error / bound; the last test writes the worst
per (op, family) into the file PCM_GEOMETRY_RECORD names
(profiles/geometry/pytest_geometry_gpu.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

import dcd_restated as D
import fscore_restated as FS
import geometry_cases as G
import kernel_loss_restated as K
import knn_restated as KN
import sliced_restated as SL
import uniform_restated as U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DCD_TOL = 1e-5  # tests/test_dcd_gpu.py's tolerance of a gradient against the oracle's chamfer_backward
_worst = {}


def _ids(op):
    return [G.entry_id(e) for e in G.entries(op)]


def _planes(t):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _like(t, lay):
    return torch.full_like(t, -7.0) if lay == 0 else torch.full_like(t.transpose(1, 2), -7.0).transpose(1, 2)


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.array(a)).to(cuda) for a in arrays]


def _ratio(err, bound):
    err = np.asarray(err, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)), initial=0.0))


def _within(op, family, what, got, want, bound):
    """|got - want| <= bound elementwise; prints and keeps the largest error / bound."""
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = _ratio(err, bound)
    print(f"  {op} {family} {what}: largest error {float(np.max(err, initial=0.0)):.3g}, error / bound {ratio:.3g}")
    _worst[(op, family)] = max(_worst.get((op, family), 0.0), ratio)
    assert (err <= bound).all(), (op, family, what, ratio)


def _exact(op, family):
    _worst.setdefault((op, family), 0.0)


def _same(first, second, what):
    for k, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(_bits(a), _bits(b)), (what, k)


def _thrice(op, family, shape, cuda, run):
    """run(case, x) -> tuple of output tensors.  The case, then another family through the same cached
    workspace, then the case again: the same bits; for `generator` once more with x as a planes view."""
    c = G.case(op, family, shape)
    first = run(c, _dev(cuda, c.x)[0])
    o = G.case(op, G.other_family(op, family), shape)
    run(o, _dev(cuda, o.x)[0])
    _same(first, run(c, _dev(cuda, c.x)[0]), (op, family, "second run"))
    if family == "generator":
        _same(first, run(c, _planes(_dev(cuda, c.x)[0])), (op, family, "planes"))
    return c, first


# ---------------------------------------------------------------------------
# kNN and the repulsion loss
# ---------------------------------------------------------------------------
def _knn(q, r, k):
    import pcm_hip
    dist = torch.full((q.shape[0], q.shape[1], k), -7.0, device=q.device)
    idx = torch.full((q.shape[0], q.shape[1], k), -7, dtype=torch.int32, device=q.device)
    pcm_hip.knn(q, pcm_hip.cloud_layout(q), r, pcm_hip.cloud_layout(r), k, dist, idx)
    return dist, idx


@pytest.mark.parametrize("entry", G.entries("knn"), ids=_ids("knn"))
def test_knn_lists_equal_the_restatement(cuda, entry):
    family, shape = entry
    want_d, want_i = G.knn_reference(family)
    for k in G.KNN_KS:
        c, (dist, idx) = _thrice("knn", family, shape, cuda, lambda c, x: _knn(x, _dev(cuda, c.y)[0], k))
        np.testing.assert_array_equal(idx.cpu().numpy(), want_i[:, :, :k], err_msg=f"{family} k={k}")
        np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), want_d[:, :, :k].view(np.int32),
                                      err_msg=f"{family} k={k}")
    _exact("knn", family)


def _repulsion(c, x):
    import pcm_hip
    lay = pcm_hip.cloud_layout(x)
    loss = torch.full((1,), -7.0, device=x.device)
    grad = _like(x, lay)
    pcm_hip.repulsion_loss(x, lay, G.REPULSION_H * c.s * c.s, loss, grad)
    return loss, grad


@pytest.mark.parametrize("entry", G.entries("repulsion"), ids=_ids("repulsion"))
def test_repulsion_loss_and_gradient(cuda, entry):
    family, shape = entry
    c, (loss, grad) = _thrice("repulsion", family, shape, cuda, _repulsion)
    h = G.REPULSION_H * c.s * c.s
    want, share, want_d, want_i = KN.repulsion_restated(c.x, h)
    assert share > 0
    # the double sum of the float32 terms rounded once, a factor two to spare
    _within("repulsion", family, "loss", loss.item(), want, 2.0 ** -23 * abs(want))
    dev = _dev(cuda, c.x)[0]
    dist, idx = _knn(dev, dev, 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32), want_d.view(np.int32))
    ref, count, mag = KN.repulsion_gradient_f64(c.x, want_d, want_i, h)
    got = grad.cpu().numpy()
    _within("repulsion", family, "gradient", got, ref, KN.gradient_bound(count, mag))
    assert (got[count == 0] == 0).all()


# ---------------------------------------------------------------------------
# FPS, the ball query and the uniform loss
# ---------------------------------------------------------------------------
def _fps(x, npoint):
    import pcm_hip
    idx = torch.full((x.shape[0], npoint), -7, dtype=torch.int64, device=x.device)
    sampled = torch.full((x.shape[0], npoint, 3), -7.0, device=x.device)
    pcm_hip.fps(x, pcm_hip.cloud_layout(x), npoint, 0, idx, sampled)
    return idx, sampled


@pytest.mark.parametrize("entry", G.entries("fps"), ids=_ids("fps"))
def test_fps_seeds_equal_the_restatement(cuda, entry):
    family, shape = entry
    c, (idx, sampled) = _thrice("fps", family, shape, cuda, lambda c, x: _fps(x, shape[2]))
    want = G.fps_reference(family, shape)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(sampled.cpu().numpy().view(np.int32), U.gather_points(c.x, want).view(np.int32))
    _exact("fps", family)


def _ball(c, centres, radius_index, cloud=None):
    import pcm_hip
    cloud = _dev(centres.device, c.y)[0] if cloud is None else cloud
    idx = torch.full((centres.shape[0], centres.shape[1], G.BALL_NSAMPLE), -7, dtype=torch.int32, device=centres.device)
    cnt = torch.full((centres.shape[0], centres.shape[1]), -7, dtype=torch.int32, device=centres.device)
    pcm_hip.ball_query(cloud, pcm_hip.cloud_layout(cloud), centres, pcm_hip.cloud_layout(centres),
                       G.BALL_RADII[radius_index] * c.s, G.BALL_NSAMPLE, idx, cnt)
    return idx, cnt


@pytest.mark.parametrize("entry", G.entries("ball"), ids=_ids("ball"))
def test_ball_query_lists_and_counts_equal_the_restatement(cuda, entry):
    family, shape = entry
    for r in range(len(G.BALL_RADII)):
        c, (idx, cnt) = _thrice("ball", family, shape, cuda, lambda c, x: _ball(c, x, r))
        want_i, want_c, _ = G.ball_reference(family, r)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
        np.testing.assert_array_equal(cnt.cpu().numpy(), want_c)
        if family == "generator":  # the searched cloud as planes too
            both = _ball(c, _planes(_dev(cuda, c.x)[0]), r, cloud=_planes(_dev(cuda, c.y)[0]))
            _same((idx, cnt), both, "ball planes")
    _exact("ball", family)


def _uniform(c, x):
    import pcm_hip
    npoint, nsample, radius, weight, L = G.uniform_params(c)
    lay = pcm_hip.cloud_layout(x)
    loss = torch.full((1,), -7.0, device=x.device)
    grad = _like(x, lay)
    groups = torch.full((x.shape[0], npoint, sum(nsample)), -7, dtype=torch.int32, device=x.device)
    pcm_hip.uniform_loss(x, lay, npoint, nsample, radius, weight, L, loss, grad, groups)
    return loss, grad, groups


@pytest.mark.parametrize("entry", G.entries("uniform"), ids=_ids("uniform"))
def test_uniform_loss_groups_loss_and_gradient(cuda, entry):
    family, shape = entry
    c, (loss, grad, groups) = _thrice("uniform", family, shape, cuda, _uniform)
    res, (ref, count, mag) = G.uniform_reference(family)
    np.testing.assert_array_equal(groups.cpu().numpy(), np.concatenate(res["groups"], axis=2))
    # one float32 rounding, a factor two to spare, as tests/test_uniform_gpu.py bounds it
    _within("uniform", family, "loss", loss.item(), res["loss"], 2.0 ** -23 * abs(res["loss"]))
    got = grad.cpu().numpy()
    _within("uniform", family, "gradient", got, ref, U.gradient_bound(count, mag))
    assert (got[count == 0] == 0).all()


# ---------------------------------------------------------------------------
# the kernel norms
# ---------------------------------------------------------------------------
def _kernel(c, x, kernel, cuda):
    import pcm_hip
    y = _dev(cuda, c.y)[0]
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((x.shape[0],), -7.0, device=cuda)
    g1, g2 = _like(x, l1), _like(y, l2)
    pcm_hip.kernel_loss(x, l1, y, l2, kernel, G.KERNEL_BLUR * c.s, loss, g1, g2)
    return loss, g1, g2


@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.KERNEL_NAMES.get)
@pytest.mark.parametrize("entry", G.entries("kernel"), ids=_ids("kernel"))
def test_kernel_loss_and_gradients_within_the_bounds(cuda, entry, kernel):
    family, shape = entry
    op = "kernel_" + K.KERNEL_NAMES[kernel]
    c, (loss, g1, g2) = _thrice("kernel", family, shape, cuda, lambda c, x: _kernel(c, x, kernel, cuda))
    n, m = c.x.shape[1], c.y.shape[1]
    want_l, want_gx, want_gy = G.kernel_reference(family, shape, kernel)
    bl = K.loss_bound(kernel, n, m, K.diameter(c.x, c.y))
    bx, by = K.grad_bound(kernel, n, m, G.KERNEL_BLUR * c.s)
    _within(op, family, "loss", loss.cpu().numpy(), want_l, bl)
    _within(op, family, "grad x", g1.cpu().numpy(), want_gx, bx)
    _within(op, family, "grad y", g2.cpu().numpy(), want_gy, by)
    if family == "identical":
        assert loss.abs().max().item() <= bl and g1.abs().max().item() <= bx and g2.abs().max().item() <= by


# ---------------------------------------------------------------------------
# Sinkhorn
# ---------------------------------------------------------------------------
def _sinkhorn(c, x, cuda):
    import pcm_hip
    y = _dev(cuda, c.y)[0]
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((x.shape[0],), -7.0, device=cuda)
    g1, g2 = _like(x, l1), _like(y, l2)
    pots = torch.full((x.shape[0], x.shape[1] + y.shape[1], 2), -7.0, device=cuda)
    pcm_hip.sinkhorn_loss(x, l1, y, l2, G.SINKHORN_BLUR * c.s, G.SINKHORN_SCALING, G.diameter(c), loss, g1, g2, pots)
    return loss, g1, g2, pots


@pytest.mark.parametrize("entry", G.entries("sinkhorn"), ids=_ids("sinkhorn"))
def test_sinkhorn_loss_gradients_and_potentials_within_tolerance(cuda, entry):
    family, shape = entry
    c, (loss, g1, g2, pots) = _thrice("sinkhorn", family, shape, cuda, lambda c, x: _sinkhorn(c, x, cuda))
    n, m = c.x.shape[1], c.y.shape[1]
    ref = G.sinkhorn_reference(family, shape)
    want_l, want_gx, want_gy, want_p = ref["ref"]
    tol_l, tol_g, tol_p = ref["tol"]
    print(f"sinkhorn {family} {shape}: diameter {ref['diameter']:.6g}, tolerances {tol_l:.3g} {tol_g:.3g} {tol_p:.3g}")
    _within("sinkhorn", family, "loss", loss.cpu().numpy(), want_l, tol_l)
    _within("sinkhorn", family, "n grad x", n * g1.cpu().numpy().astype(np.float64), n * want_gx, tol_g)
    _within("sinkhorn", family, "m grad y", m * g2.cpu().numpy().astype(np.float64), m * want_gy, tol_g)
    _within("sinkhorn", family, "potentials", pots.cpu().numpy(), want_p, tol_p)
    if family == "identical":
        assert loss.abs().max().item() <= tol_l
        assert n * g1.abs().max().item() <= tol_g and m * g2.abs().max().item() <= tol_g


# ---------------------------------------------------------------------------
# sliced Wasserstein
# ---------------------------------------------------------------------------
def _sliced(c, x, dirs, cuda):
    import pcm_hip
    y, dd = _dev(cuda, c.y, dirs)
    b, n, m, l = x.shape[0], x.shape[1], y.shape[1], dd.shape[0]
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((b,), -7.0, device=cuda)
    slices = torch.full((b, l), -7.0, device=cuda)
    g1, g2 = _like(x, l1), _like(y, l2)
    o1 = torch.full((b, l, n), -7, dtype=torch.int32, device=cuda)
    o2 = torch.full((b, l, m), -7, dtype=torch.int32, device=cuda)
    pcm_hip.sliced_wasserstein_loss(x, l1, y, l2, dd, loss, slices, g1, g2, o1, o2)
    return loss, slices, g1, g2, o1, o2


@pytest.mark.parametrize("entry", G.entries("sliced"), ids=_ids("sliced"))
def test_sliced_orders_equal_and_values_within_bounds(cuda, entry):
    family, shape = entry
    dirs, results = G.sliced_reference(family, shape)
    c, (loss, slices, g1, g2, o1, o2) = _thrice("sliced", family, shape, cuda, lambda c, x: _sliced(c, x, dirs, cuda))
    n, m, l = c.x.shape[1], c.y.shape[1], shape[3]
    for bi, res in enumerate(results):
        assert np.array_equal(o1[bi].cpu().numpy(), res["order1"]), (entry, bi, "order1")
        assert np.array_equal(o2[bi].cpu().numpy(), res["order2"]), (entry, bi, "order2")
        bl, bs, bx, by = SL.bounds(n, m, l, res, dirs)
        _within("sliced", family, f"element {bi} loss", loss[bi].item(), res["loss"], bl)
        _within("sliced", family, f"element {bi} slices", slices[bi].cpu().numpy(), res["slices"], bs)
        _within("sliced", family, f"element {bi} grad x", g1[bi].cpu().numpy(), res["gx"], bx)
        _within("sliced", family, f"element {bi} grad y", g2[bi].cpu().numpy(), res["gy"], by)
    if family == "identical":  # every bound is 0 there: exactly 0
        assert not loss.any() and not slices.any() and not g1.any() and not g2.any()


# ---------------------------------------------------------------------------
# DCD
# ---------------------------------------------------------------------------
def _dcd(c, x, alpha, lam, cuda):
    import pcm_hip
    y = _dev(cuda, c.y)[0]
    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((b,), -7.0, device=cuda)
    cd = torch.full((b, 2), -7.0, device=cuda)
    g1, g2 = _like(x, l1), _like(y, l2)
    c1 = torch.full((b, n), -7, dtype=torch.int32, device=cuda)
    c2 = torch.full((b, m), -7, dtype=torch.int32, device=cuda)
    gd1, gd2 = torch.full((b, n), -7.0, device=cuda), torch.full((b, m), -7.0, device=cuda)
    pcm_hip.dcd_loss(x, l1, y, l2, float(alpha), float(lam), False, loss, cd, g1, g2, c1, c2, gd1, gd2)
    return loss, cd, g1, g2, c1, c2, gd1, gd2


@pytest.mark.parametrize("lam", G.DCD_LAMBDAS, ids=lambda v: f"lambda{v}")
@pytest.mark.parametrize("entry", G.entries("dcd"), ids=_ids("dcd"))
def test_dcd_counts_equal_and_values_within_bounds(cuda, oracle, entry, lam):
    family, shape = entry
    d1, d2, i1, i2, alpha = G.dcd_forward(family, shape)
    # the other family's call takes its own alpha: median_alpha goes with the cloud
    c, out = _thrice("dcd", family, shape, cuda,
                     lambda c, x: _dcd(c, x, G.dcd_forward(c.family, c.shape)[4], lam, cuda))
    loss, cd, g1, g2, c1, c2, gd1, gd2 = (t.cpu().numpy() for t in out)
    b, n, m = shape[0], c.x.shape[1], c.y.shape[1]
    res = G.dcd_reference(family, shape, lam)
    assert np.array_equal(c1, res["c1"]) and np.array_equal(c2, res["c2"])
    assert c1.sum() == b * m and c2.sum() == b * n
    bl, bc, b1, b2 = D.bounds(res, alpha, lam, n, m)
    _within("dcd", family, "loss", loss, res["loss"], bl)
    _within("dcd", family, "cd", cd, res["cd"], bc)
    _within("dcd", family, "graddist1", gd1, res["gd1"], b1)
    _within("dcd", family, "graddist2", gd2, res["gd2"], b2)
    # the gradients: the oracle's deterministic backward on the call's own graddists
    # at DCD_TOL carried to the case's gradient size (never above DCD_TOL: a small gradient is not let off)
    r1, r2 = oracle.chamfer_backward(c.x, c.y, gd1, gd2, i1, i2)
    t1, t2 = G.dcd_gradient_tolerance(family, shape, lam, DCD_TOL)
    for name, value, want, tol in (("gradxyz1", g1, r1, t1), ("gradxyz2", g2, r2, t2)):
        err = float(np.abs(value - want).max())
        print(f"  dcd {family} {name}: largest error {err:.3g} (tolerance {tol:.3g}, largest |gradient| "
              f"{float(np.abs(want).max()):.3g})")
        assert tol <= DCD_TOL
        np.testing.assert_allclose(value, want, rtol=0, atol=tol)
    if family == "collapsed":
        assert (c1[:, 0] == m).all() and not c1[:, 1:].any()
    if family == "identical":  # d = 0 and a count of 1 for every query: one graddist, that of d = 0
        assert not d1.any() and not d2.any() and (c1 == 1).all() and (c2 == 1).all()
        zero = D.evaluate(np.zeros_like(d1), np.zeros_like(d2), i1, i2, alpha, lam, False)
        assert np.array_equal(zero["gd1"], res["gd1"])
        assert len(np.unique(gd1)) == 1 and len(np.unique(gd2)) == 1


# ---------------------------------------------------------------------------
# F-score: the one-pass Chamfer evaluation
# ---------------------------------------------------------------------------
def _fscore(c, cuda, rows=slice(None)):
    """pcm_chamfer_eval on the case (or on `rows` of its batch) at the case's thresholds -> numpy
    (mean_dist [B,2], counts [B,T,2], scores [B,T,3], batch [T,3])."""
    import pcm_hip
    x, y = _dev(cuda, c.x[rows], c.y[rows])
    ths = G.fscore_thresholds(c)
    b, t = x.shape[0], len(ths)
    md = torch.full((b, 2), -7.0, device=cuda)
    cn = torch.full((b, t, 2), -7, dtype=torch.int32, device=cuda)
    sc = torch.full((b, t, 3), -7.0, device=cuda)
    bs = torch.full((t, 3), -7.0, device=cuda)
    pcm_hip.chamfer_eval(x, y, ths, md, cn, sc, bs)
    torch.cuda.synchronize()
    return md.cpu().numpy(), cn.cpu().numpy(), sc.cpu().numpy(), bs.cpu().numpy()


def _fscore_check(family, shape, cuda, oracle):
    c = G.case("fscore", family, shape)
    if shape in G.SHAPES["fscore"]:
        d1, d2 = G.fscore_forward(family, shape)
    else:  # the one wide case: not kept
        d1, d2, _, _ = oracle.chamfer_forward(c.x, c.y)
    ths = G.fscore_thresholds(c)
    n, m = c.x.shape[1], c.y.shape[1]
    md, cn, sc, bs = first = _fscore(c, cuda)
    _fscore(G.case("fscore", G.other_family("fscore", family), shape), cuda)  # through the cached workspace
    for k, (a, b) in enumerate(zip(first, _fscore(c, cuda))):
        assert np.array_equal(FS.bits(a), FS.bits(b)), (family, shape, "second run", k)
    np.testing.assert_array_equal(cn[:, :, 0], FS.counts_from(d1, ths))
    np.testing.assert_array_equal(cn[:, :, 1], FS.counts_from(d2, ths))
    want = FS.scores_from(cn[:, :, 0], cn[:, :, 1], n, m)
    np.testing.assert_array_equal(FS.bits(sc), FS.bits(want))
    np.testing.assert_array_equal(FS.bits(bs), FS.bits(FS.batch_from(want)))
    # rtol 1e-5 (167 x 2^-24) of the float64 mean: non-negative terms, chains of at most 6 DPP steps + 8 waves
    # + 20 records (a workgroup per 128 or 256 queries) -- as tests/test_fscore_gpu.py derives it; where the
    # quotient rounds in the subnormal range, half a subnormal's spacing more (2^-149 covers it)
    ref = np.stack([d1.astype(np.float64).mean(1), d2.astype(np.float64).mean(1)], 1)
    if family == "identical":
        assert not md.any() and not ref.any()
    _within("fscore", family, "mean_dist", md, ref, 1e-5 * ref + (2.0 ** -149 if family == "scale_1e-20" else 0.0))
    return c, first


@pytest.mark.parametrize("entry", G.entries("fscore"), ids=_ids("fscore"))
def test_fscore_counts_equal_scores_bitwise_and_means_within_bound(cuda, oracle, entry):
    _fscore_check(entry[0], entry[1], cuda, oracle)


@pytest.mark.parametrize("family", ["centred", "offset_1000"])
def test_fscore_four_queries_per_lane(cuda, oracle, family):
    _fscore_check(family, G.FSCORE_WIDE_SHAPE, cuda, oracle)


def test_fscore_subnormal_cloud_alone_equals_its_place_in_the_batch(cuda, oracle):
    shape = G.SHAPES["fscore"][1]
    c = G.case("fscore", "scale_1e-20", shape)
    md, cn, sc, _ = _fscore(c, cuda)
    md1, cn1, sc1, bs1 = _fscore(c, cuda, rows=slice(1, 2))
    assert cn1[0, :3].min() > 0 and cn1[0, 0].max() < cn1[0, 2].min()  # the subnormal thresholds do count
    np.testing.assert_array_equal(cn1[0], cn[1])
    np.testing.assert_array_equal(FS.bits(md1[0]), FS.bits(md[1]))
    np.testing.assert_array_equal(FS.bits(sc1[0]), FS.bits(sc[1]))
    np.testing.assert_array_equal(FS.bits(bs1), FS.bits(sc[1]))  # a batch of one: its own scores


# ---------------------------------------------------------------------------
# power-of-two scaling, and the record
# ---------------------------------------------------------------------------
def test_scaling_by_1024_keeps_seeds_lists_and_orders(cuda):
    for shape in G.SHAPES["fps"]:
        unit, big = (_fps(_dev(cuda, G.case("fps", f, shape).x)[0], shape[2])[0] for f in ("unit", "scale_1024"))
        assert torch.equal(unit, big)
        np.testing.assert_array_equal(unit.cpu().numpy(), G.fps_reference("unit", shape))
    shape = G.SHAPES["knn"][0]
    lists = []
    for f in ("unit", "scale_1024"):
        c = G.case("knn", f, shape)
        lists.append(_knn(*_dev(cuda, c.x, c.y), max(G.KNN_KS)))
    assert torch.equal(lists[0][1], lists[1][1]) and torch.equal(_bits(lists[0][0] * 2.0 ** 20), _bits(lists[1][0]))
    np.testing.assert_array_equal(lists[0][1].cpu().numpy(), G.knn_reference("unit")[1])
    for shape in G.SHAPES["sliced"]:
        dirs = G.sliced_dirs(shape[3])
        orders = []
        for f in ("unit", "scale_1024"):
            c = G.case("sliced", f, shape)
            orders.append(_sliced(c, _dev(cuda, c.x)[0], dirs, cuda)[4:])
        _same(orders[0], orders[1], "sliced orders")
        assert np.array_equal(orders[0][0][0].cpu().numpy(), G.sliced_reference("unit", shape)[1][0]["order1"])
    shape = G.SHAPES["ball"][0]
    for r in range(len(G.BALL_RADII)):
        got = []
        for f in ("unit", "scale_1024"):
            c = G.case("ball", f, shape)
            got.append(_ball(c, _dev(cuda, c.x)[0], r))
        _same(got[0], got[1], "ball query")
        np.testing.assert_array_equal(got[0][0].cpu().numpy(), G.ball_reference("unit", r)[0])


def test_record_largest_ratio():
    """After the comparisons above (same process): the figures for profiles/geometry/."""
    print("largest error / bound:", _worst)
    if os.environ.get("PCM_GEOMETRY_RECORD") and _worst:
        path = os.path.join(REPO, os.environ["PCM_GEOMETRY_RECORD"])
        with open(path, "w") as f:
            f.write(f"tests/test_geometry_gpu.py on {torch.cuda.get_device_name(0)}\n"
                    "largest error / bound per (op, family); 0 for the outputs compared for equality "
                    "(indices, counts, orders, distance bits: equal in all):\n")
            for (op, family), v in sorted(_worst.items()):
                f.write(f"  {op} {family}: {v:.4g}\n")
