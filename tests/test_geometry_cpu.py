"""tests/geometry_cases.py checked without a GPU: every family does what its
row of the table claims (on the restatement), the float32 restatements stay
inside the bounds the GPU comparison uses on every case, the modelled defects
of each module still leave those bounds, the two assumptions behind
kernel_loss_restated.grad_bound and dcd_restated's RHO hold or are covered,
scaling by 1024 keeps the index outputs bit for bit, and the ninth op's
(F-score: the one-pass Chamfer evaluation) thresholds separate the points of
every family, across subnormal distances and exact ties where the table says so."""
import numpy as np
import pytest

import dcd_restated as D
import fscore_restated as FS
import geometry_cases as G
import kernel_loss_restated as K
import sinkhorn_restated as S
import sliced_restated as SL
import uniform_restated as U

TINY = np.float32(2.0 ** -126)


def _ids(op):
    return [G.entry_id(e) for e in G.entries(op)]


# ---------------------------------------------------------------------------
# the inputs do what the table claims
# ---------------------------------------------------------------------------
def test_every_op_takes_the_families_of_the_table():
    assert len(G.GENERAL) == 12 and set(G.GENERAL) <= set(G.TRANSFORMS)
    for op, families in G.FAMILIES.items():
        assert set(G.GENERAL) - {"identical", "far_point", "bimodal"} <= set(families)
        assert set(families) <= set(G.GENERAL) | {"scale_2e5", "scale_1e-20", "offset_duplicates"}
        assert ("scale_2e5" in families) == (op == "fps")
        assert ("scale_1e-20" in families) == (op in ("fps", "ball", "fscore"))
    for op in G.FAMILIES:
        for family, shape in G.entries(op):
            c, u = G.case(op, family, shape), G.case(op, "unit", shape)
            if family not in ("identical",):
                assert c.x.shape == u.x.shape and c.y.shape == u.y.shape
            assert c.x.dtype == np.float32 and c.y.dtype == np.float32
            # no family is the plain unit-cube pair
            assert not (np.array_equal(c.x, u.x) and np.array_equal(c.y, u.y)), (op, family)
    x, y = G.case("kernel", "centred", (2, 257, 255))[3:5]
    assert x.min() < -0.4 and y.min() > 0.2 and x.max() < 0.5
    x, y = G.case("sinkhorn", "generator", (2, 127, 128))[3:5]
    assert x.min() < -1.4 and x.max() > 1.4 and y.min() >= 0.75 and K.diameter(x, y) ** 2 > 20
    c = G.case("dcd", "duplicates", (2, 1000, 333))
    assert np.array_equal(c.x[:, 500:], c.x[:, :500]) and np.array_equal(c.y[:, 167:], c.y[:, :166])
    c = G.case("knn", "far_point", (2, 300, 1025))
    assert (c.y[:, 7] == np.array([30, -30, 30], np.float32)).all()
    c = G.case("sliced", "identical", (2, 1000, 333, 65))
    assert c.x.shape == c.y.shape == (2, 1000, 3) and np.array_equal(c.x, c.y) and c.x is not c.y


@pytest.mark.parametrize("shape", G.SHAPES["fps"], ids=str)
def test_fps_saturated_and_subnormal_scales(shape):
    unit = G.fps_reference("unit", shape)
    d = G.fps_first_distances(G.case("fps", "scale_2e5", shape).x)
    assert (d > np.float32(1e10)).any() and ((d < np.float32(1e10)) & (d > 0)).any()
    assert not np.array_equal(G.fps_reference("scale_2e5", shape), unit)
    d = G.fps_first_distances(G.case("fps", "scale_1e-20", shape).x)
    assert ((d > 0) & (d < TINY)).sum() >= d.size - 2 * d.shape[0] and (d < TINY).all()
    assert np.array_equal(G.fps_reference("scale_1e-20", shape), unit)


def test_offset_clouds_are_quantised_and_have_exact_ties():
    """At 1000 a float32 has 2^-14 = 6.1e-5 between neighbours: every coordinate is a multiple of it, distinct
    points share coordinates exactly (dx = 0) and a query has distinct candidates at exactly equal distances.
    Measured on these clouds: 5 of 300 query rows hold such a tie, none of them inside a 32-slot list, and no two
    distinct points coincide in all three coordinates (the chance is 7e-8 for the 3e5 pairs) -- the zero
    distances between distinct indices come from `duplicates`, `collapsed` and `identical`, asserted below."""
    c = G.case("knn", "offset_1000", G.SHAPES["knn"][0])
    for cloud in (c.x, c.y):
        assert (np.abs(cloud) >= 1000).all() and not (cloud * np.float32(2 ** 14) % 1).any()
    diff = c.y[0][None, :, :] - c.x[0][:, None, :]
    assert (diff == 0).sum() >= 8 and not (diff == 0).all(-1).any()
    d = np.sort(U.sqd_pinned(diff[..., 0], diff[..., 1], diff[..., 2]), axis=1)
    assert (d[:, 1:] == d[:, :-1]).any(axis=1).sum() >= 2
    # every difference is exact: the float32 distance is the pinned sum of exact squares
    assert np.array_equal(diff.astype(np.float64), c.y[0].astype(np.float64)[None] - c.x[0].astype(np.float64)[:, None])
    dist, idx = G.knn_reference("duplicates")  # bit-equal candidates: equal distances, the lower index first
    tie = dist[:, :, 1:] == dist[:, :, :-1]
    assert tie.sum() >= dist.shape[0] * dist.shape[1] and (idx[:, :, 1:][tie] > idx[:, :, :-1][tie]).all()
    assert (G.knn_reference("identical")[0][:, :, 0] == 0).all()
    for family in ("duplicates", "collapsed", "offset_duplicates"):  # a zero distance to another index in the self search
        x = G.case("repulsion", family, G.SHAPES["repulsion"][0]).x
        assert (U.knn_restated(x, x, 5)[0][:, :, 1] == 0).sum() >= x.shape[0] * (x.shape[1] - 1)
    # offset_duplicates: the same at coordinate 1000 -- d = 0 between distinct indices, ties inside the lists,
    # a ball query whose cloud holds bit-equal points, FPS minima that reach 0 away from the seed
    assert (np.abs(x) >= 1000).all()
    dist, idx = G.knn_reference("offset_duplicates")
    tie = dist[:, :, 1:] == dist[:, :, :-1]
    assert tie.sum() >= dist.shape[0] * dist.shape[1] and (idx[:, :, 1:][tie] > idx[:, :, :-1][tie]).all()
    c = G.case("ball", "offset_duplicates", G.SHAPES["ball"][0])
    assert (np.abs(c.y) >= 1000).all() and np.array_equal(c.y[:, 129:], c.y[:, :128])
    d = G.fps_first_distances(G.case("fps", "offset_duplicates", G.SHAPES["fps"][0]).x)
    assert ((d == 0).sum(axis=1) == 2).all()


@pytest.mark.parametrize("family", ["plane", "line", "collapsed", "duplicates"])
def test_degenerate_clouds_have_runs_of_equal_sort_keys(family):
    for shape in G.SHAPES["sliced"]:
        c = G.case("sliced", family, shape)
        keys = SL.keys(SL.project(c.x[0], G.sliced_dirs(shape[3])))
        longest = max(np.unique(row, return_counts=True)[1].max() for row in keys)
        print(family, shape, "longest run of equal keys", longest)
        if family in ("plane", "line", "collapsed"):
            assert longest >= 8
        else:
            assert longest >= 2


def test_collapsed_cloud_takes_every_hit_at_index_zero(oracle):
    for shape in G.SHAPES["dcd"]:
        d1, d2, i1, i2, alpha = G.dcd_forward("collapsed", shape)
        res = G.dcd_reference("collapsed", shape, 1.0)
        m = shape[2]
        assert (i2 == 0).all() and (res["c1"][:, 0] == m).all() and (res["c1"][:, 1:] == 0).all()


def test_bimodal_exponents_underflow_across_and_not_within():
    for shape in G.SHAPES["kernel"]:
        c = G.case("kernel", "bimodal", shape)
        sigma = float(np.float32(G.KERNEL_BLUR))
        x, y = c.x[0].astype(np.float64), c.y[0].astype(np.float64)
        cross = -((x[:, None] - y[None]) ** 2).sum(-1) / (2 * sigma * sigma) / np.log(2)  # base-2 exponents
        own = -((x[:, None] - x[None]) ** 2).sum(-1) / (2 * sigma * sigma) / np.log(2)
        assert cross.min() < -150 and np.where(np.eye(len(x), dtype=bool), -np.inf, own).max() > -1
    sched = S.schedule(G.SINKHORN_BLUR, G.SINKHORN_SCALING, G.diameter(G.case("sinkhorn", "bimodal", (2, 127, 128))))
    assert 14 <= len(sched) <= 18 and sched[0] > 9e5


def test_every_ball_query_family_has_empty_partly_filled_and_over_full_balls():
    for family in G.FAMILIES["ball"]:
        kinds = set()
        for r in range(len(G.BALL_RADII)):
            hits = G.ball_reference(family, r)[2]
            kinds |= {name for name, mask in (("empty", hits == 0), ("partly", (hits > 0) & (hits < G.BALL_NSAMPLE)),
                                              ("over", hits > G.BALL_NSAMPLE)) if mask.any()}
        if family == "identical":  # the centres search themselves: d = 0 < r2 puts every centre in its own ball
            for r in range(len(G.BALL_RADII)):
                idx, cnt, hits = G.ball_reference(family, r)
                assert (hits >= 1).all() and (idx[:, :, 0] <= np.arange(idx.shape[1])[None, :]).all()
            assert kinds == {"partly"}, kinds  # 65 points over [-0.2, 1.2)^3: at most a few to a ball
        else:
            assert kinds == {"empty", "partly", "over"}, (family, kinds)
    idx = G.ball_reference("collapsed", 1)[0]
    assert (idx == idx[:, :1]).all() and len(np.unique(idx[0, 0])) > 1  # 65 equal centres: one list, 65 times
    c = G.case("ball", "scale_1e-20", G.SHAPES["ball"][0])
    r2 = np.float32(np.float32(G.BALL_RADII[1] * c.s) * np.float32(G.BALL_RADII[1] * c.s))
    assert 0 < r2 < TINY


def test_scaled_parameters_go_with_the_cloud():
    c = G.case("uniform", "scale_1e3", G.SHAPES["uniform"][0])
    u = G.case("uniform", "unit", G.SHAPES["uniform"][0])
    assert G.uniform_params(c)[2] == pytest.approx([1e3 * r for r in G.uniform_params(u)[2]])
    assert G.uniform_params(c)[4] == pytest.approx(1e3 * G.uniform_params(u)[4])
    assert G.diameter(G.case("sinkhorn", "scale_1e-3", (2, 127, 128))) == pytest.approx(1e-3 * S.DIAMETER, rel=1e-6)
    c = G.case("sinkhorn", "far_point", (2, 127, 128))
    assert G.diameter(c) == float(np.float32(K.diameter(c.x, c.y))) > 50


# ---------------------------------------------------------------------------
# F-score: the thresholds separate the points
# ---------------------------------------------------------------------------
# `identical`: every nearest distance is 0, under every positive threshold -- all counts full (asserted).
# `line`: 300 and 1025 points on one segment of length 1 are at most 2e-3 apart, squared 4e-6 < 1e-4 (but for a
# point or two past the other cloud's ends) -- the counts are full or one short at every threshold (asserted).
FSCORE_TRIVIAL = ("identical", "line")


def test_fscore_thresholds_separate_the_points_of_every_family(oracle):
    """Per family and shape the counts over the five thresholds are neither all 0 nor all full in either
    direction, and the five (count1, count2) pairs hold three distinct ones, for every family but FSCORE_TRIVIAL."""
    assert set(G.FAMILIES["fscore"]) == set(G.GENERAL) | {"scale_1e-20", "offset_duplicates"}
    assert G.SHAPES["fscore"] == [(2, 300, 1025), (2, 2048, 2047)]  # 2 queries per lane; on and one below the tile
    for family, shape in G.entries("fscore"):
        c = G.case("fscore", family, shape)
        b, n, m = shape[0], c.x.shape[1], c.y.shape[1]
        th = G.fscore_thresholds(c)
        assert len(th) == 5 and all(np.float32(t) == t and t > 0 for t in th)
        d1, d2 = G.fscore_forward(family, shape)
        assert d1.shape == (b, n) and d2.shape == (b, m) and d1.dtype == np.float32
        c1, c2 = FS.counts_from(d1, th).sum(0), FS.counts_from(d2, th).sum(0)
        print(family, shape, c1.tolist(), c2.tolist())
        if family == "identical":
            assert not d1.any() and not d2.any() and (c1 == b * n).all() and (c2 == b * m).all()
        elif family == "line":
            assert (c1 >= b * n - 2).all() and (c2 >= b * m - 2).all()
        else:
            for cnt, full in ((c1, b * n), (c2, b * m)):
                assert not (cnt == 0).all() and not (cnt == full).all(), (family, shape)
                assert len(np.unique(cnt)) >= 2, (family, shape, cnt)
            # three distinct (count1, count2) pairs: `collapsed` has two values in its first direction alone
            assert len(set(zip(c1.tolist(), c2.tolist()))) >= 3, (family, shape)
    for family in ("centred", "offset_1000"):  # the 4-queries-per-lane case
        c = G.case("fscore", family, G.FSCORE_WIDE_SHAPE)
        assert c.x.shape == (64, 1030, 3) and c.y.shape == (64, 700, 3)
        assert 64 * ((1030 + 255) // 256 + (700 + 255) // 256) >= 512  # eval_qpt's switch


def test_fscore_subnormal_distances_straddle_subnormal_thresholds(oracle):
    """scale_1e-20: every nearest distance is a float32 subnormal (or 0), the first three thresholds are
    subnormal, and at least two thresholds have subnormal distances on both sides."""
    for shape in G.SHAPES["fscore"]:
        c = G.case("fscore", "scale_1e-20", shape)
        th = np.float32(G.fscore_thresholds(c))
        assert (th[:3] < TINY).all() and (th > 0).all() and th[4] < TINY
        d = np.concatenate([v.ravel() for v in G.fscore_forward("scale_1e-20", shape)])
        sub = (d > 0) & (d < TINY)
        print(shape, "subnormal", int(sub.sum()), "zero", int((d == 0).sum()), "of", d.size)
        assert (d < TINY).all() and sub.sum() >= d.size - 2
        straddled = [t for t in th if (d[sub] < t).any() and (d[sub] >= t).any()]
        assert len(straddled) >= 2, straddled
        # subnormals are multiples of 2^-149 and the first threshold is 7 of them: distances bit-equal to a
        # threshold exist, and the strict count leaves them out
        d1 = G.fscore_forward("scale_1e-20", shape)[0]
        equal = (d1[:, None, :] == th[None, :, None]).sum(-1)
        assert equal[:, :3].sum() >= 1, equal
        assert np.array_equal(FS.counts_from(d1, th), d1.shape[1] - (d1[:, None, :] >= th[None, :, None]).sum(-1))
        # the counts are the unit pair's but for the quantisation of a subnormal: they move by a few points
        unit = G.case("fscore", "unit", shape)
        want = FS.counts_from(G.fscore_forward("unit", shape)[0], G.fscore_thresholds(unit)).sum(0)
        got = FS.counts_from(G.fscore_forward("scale_1e-20", shape)[0], th).sum(0)
        assert np.abs(got - want).max() <= 0.02 * d.size and (got[3:] == want[3:]).all()


def test_fscore_offset_cloud_has_bit_equal_candidates(oracle):
    """offset_1000: coordinates quantised to 2^-14, so a query meets distinct candidates at bit-equal pinned
    distances; the scan's minimum does not depend on which of them it meets first.  offset_duplicates: the
    nearest distance itself is attained twice."""
    shape = G.SHAPES["fscore"][0]
    c = G.case("fscore", "offset_1000", shape)
    diff = c.y[0][None, :, :] - c.x[0][:, None, :]
    d = np.sort(U.sqd_pinned(diff[..., 0], diff[..., 1], diff[..., 2]), axis=1)
    assert (d[:, 1:] == d[:, :-1]).any(axis=1).sum() >= 2
    assert np.array_equal(d[:, 0].view(np.int32), G.fscore_forward("offset_1000", shape)[0][0].view(np.int32))
    c = G.case("fscore", "offset_duplicates", shape)
    diff = c.y[0][None, :, :] - c.x[0][:, None, :]
    d = np.sort(U.sqd_pinned(diff[..., 0], diff[..., 1], diff[..., 2]), axis=1)
    assert (d[:, 0] == d[:, 1]).sum() >= 0.9 * d.shape[0]


# ---------------------------------------------------------------------------
# the assumptions behind two bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", G.entries("kernel"), ids=_ids("kernel"))
def test_no_kernel_loss_case_has_a_difference_whose_square_underflows(entry):
    """kernel_loss_restated.grad_bound leaves out a difference whose square underflows float32: every non-zero
    coordinate difference of every case squares to a normal float32 (scale_1e-3 is the nearest: 1e-21)."""
    c = G.case("kernel", *entry)
    for p, q in ((c.x, c.x), (c.y, c.y), (c.x, c.y)):
        for bi in range(p.shape[0]):
            d = (p[bi][:, None, :] - q[bi][None, :, :]).astype(np.float32)
            sq = (d * d)[d != 0]
            assert sq.size == 0 or sq.min() >= TINY


def test_dcd_terms_beyond_the_argued_range_are_exactly_zero_in_both_precisions(oracle):
    """dcd_restated's RHO is argued for a = alpha d < 16000 and extended beyond in its docstring: there e = 0,
    g = 0, term = 1 and graddist = 0 exactly in float32 and in float64, so RHO multiplies nothing."""
    beyond = 0
    for family, shape in G.entries("dcd"):
        d1, d2, i1, i2, alpha = G.dcd_forward(family, shape)
        for lam in G.DCD_LAMBDAS:
            res = G.dcd_reference(family, shape, lam)
            f32 = D.evaluate(d1, d2, i1, i2, alpha, lam, False, dtype=np.float32)
            for tag in "12":
                far = res["a" + tag] >= 16000
                beyond += int(far.sum())
                for r in (res, f32):
                    assert np.isfinite(r["a" + tag]).all()
                    assert (r["g" + tag][far] == 0).all() and (r["term" + tag][far] == 1).all()
                    assert (r["gd" + tag][far] == 0).all()
        if family != "far_point":
            assert not (res["a1"] >= 16000).any() and not (res["a2"] >= 16000).any(), family
    assert beyond >= 2 * 2 * len(G.DCD_LAMBDAS)  # far_point's outlier, every element, shape and lambda


# ---------------------------------------------------------------------------
# the float32 restatements stay inside the bounds; the modelled defects leave them
# ---------------------------------------------------------------------------
def _sinkhorn_moved(full, cut, n, m, tol, skip_rows=None):
    dl = abs(S.loss_from(cut, skip_rows) - S.loss_from(full))
    if not dl <= 10 * tol[0]:
        return True
    if cut["weights"] is None:
        return False
    (gx, gy), (hx, hy) = S.grads_from(full), S.grads_from(cut)
    return max(n * np.abs(hx - gx).max(), m * np.abs(hy - gy).max()) > 10 * tol[1]


@pytest.mark.parametrize("entry", G.entries("sinkhorn"), ids=_ids("sinkhorn"))
def test_sinkhorn_tolerances_are_held_by_both_conditions(entry):
    """(a) the float32 restatement is within a quarter of the scaled tolerances, or the case's tolerance is four
    times its own error (geometry_cases.sinkhorn_reference; which of the two is printed); (b) against that
    tolerance a left-out schedule entry (one of the last three), the first tile of columns of either cloud left
    out of the cross softmins and the first block of rows of either cloud left out of the loss each move the
    float64 result by more than ten tolerances.  With identical clouds every row's term F_cross - F_own is 0,
    so a left-out block of rows or schedule entry cannot show; the left-out columns do."""
    family, shape = entry
    ref = G.sinkhorn_reference(family, shape)
    c = G.case("sinkhorn", family, shape)
    n, m = c.x.shape[1], c.y.shape[1]
    print(entry, "float32 error / scaled tolerance: loss %.3g grad %.3g pot %.3g" % tuple(
        e / t for e, t in zip(ref["err32"], ref["scaled"])), "diameter %.4g" % ref["diameter"])
    for e, t, s in zip(ref["err32"], ref["tol"], ref["scaled"]):
        assert e <= 0.25 * t and (t == s or t == 4 * e)
        assert t == s or e > 0.25 * s or family in G.SINKHORN_OWN_ERROR  # the scaled one wherever it holds both
    eps = S.schedule(ref["blur"], G.SINKHORN_SCALING, ref["diameter"])
    full = S.sinkhorn_one(c.x[0], c.y[0], eps)
    tol = ref["tol"]
    for cloud, cnt in ((0, n), (1, m)):
        cut = S.sinkhorn_one(c.x[0], c.y[0], eps, skip_cols=(cloud, 0, min(S.TILE, cnt)))
        assert _sinkhorn_moved(full, cut, n, m, tol), (entry, "columns", cloud)
        if family != "identical":
            assert _sinkhorn_moved(full, full, n, m, tol, skip_rows=(cloud, 0, min(S.ROWS, cnt))), (entry, "rows", cloud)
    if family != "identical":
        for k in range(len(eps) - 3, len(eps)):
            assert _sinkhorn_moved(full, S.sinkhorn_one(c.x[0], c.y[0], eps[:k] + eps[k + 1:]), n, m, tol), (entry, "entry", k)


def test_sinkhorn_leaves_bimodal_out_because_no_tolerance_holds_both_conditions():
    """The one family the Sinkhorn comparison drops: with the scaled tolerances, and with four times the float32
    restatement's own error as well, a left-out schedule entry moves the float64 result by less than ten
    tolerances.  And far_point's narrower tolerance is needed: with the scaled one the last entry falls short."""
    assert "bimodal" not in G.FAMILIES["sinkhorn"] and len(G.FAMILIES["sinkhorn"]) == len(G.GENERAL) - 1
    shape = G.SHAPES["sinkhorn"][0]
    ref = G.sinkhorn_reference("bimodal", shape)
    c = G.case("sinkhorn", "bimodal", shape)
    n, m = c.x.shape[1], c.y.shape[1]
    eps = S.schedule(ref["blur"], G.SINKHORN_SCALING, ref["diameter"])
    full = S.sinkhorn_one(c.x[0], c.y[0], eps)
    own = tuple(4 * e for e in ref["err32"])
    cut = S.sinkhorn_one(c.x[0], c.y[0], eps[:-1])
    assert not _sinkhorn_moved(full, cut, n, m, ref["scaled"]) and not _sinkhorn_moved(full, cut, n, m, own)
    shape = G.SHAPES["sinkhorn"][1]
    ref = G.sinkhorn_reference("far_point", shape)
    c = G.case("sinkhorn", "far_point", shape)
    eps = S.schedule(ref["blur"], G.SINKHORN_SCALING, ref["diameter"])
    full, cut = S.sinkhorn_one(c.x[0], c.y[0], eps), S.sinkhorn_one(c.x[0], c.y[0], eps[:-1])
    assert not _sinkhorn_moved(full, cut, 300, 1025, ref["scaled"]) and _sinkhorn_moved(full, cut, 300, 1025, ref["tol"])
    assert all(t < s for t, s in zip(ref["tol"], ref["scaled"]))


def _sliced_ratios(n, m, l, res, other, dirs):
    bl, bs, bx, by = SL.bounds(n, m, l, res, dirs)

    def ratio(err, bound):
        bound = np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
        with np.errstate(invalid="ignore"):
            return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)), initial=0.0))

    return (ratio(np.abs(np.float64(other["loss"]) - res["loss"]), bl),
            ratio(np.abs(other["slices"].astype(np.float64) - res["slices"]), bs),
            ratio(np.abs(other["gx"].astype(np.float64) - res["gx"]), bx),
            ratio(np.abs(other["gy"].astype(np.float64) - res["gy"]), by))


@pytest.mark.parametrize("entry", G.entries("sliced"), ids=_ids("sliced"))
def test_sliced_float32_restatement_and_defects(entry):
    """The float32 evaluation within a quarter of sliced_restated.bounds on every case; the dropped last
    direction and (n not dividing m) the floor defect leave them by more than ten bounds; ties ordered by
    descending index change an order array wherever the family has equal keys.  Identical clouds have every
    output and every bound 0: only the orders can differ there."""
    family, shape = entry
    c = G.case("sliced", family, shape)
    b, n, m, l = shape[0], c.x.shape[1], c.y.shape[1], shape[3]
    dirs, results = G.sliced_reference(family, shape)
    for bi in range(b):
        f32 = SL.sliced_one(c.x[bi], c.y[bi], dirs, dtype=np.float32)
        figures = _sliced_ratios(n, m, l, results[bi], f32, dirs)
        assert max(figures) <= 0.25, (entry, bi, figures)
    res = results[0]
    if family == "identical":
        assert res["loss"] == 0 and not res["gx"].any() and not res["gy"].any() and res["D"] == 0
    else:
        bad = SL.sliced_one(c.x[0], c.y[0], dirs, drop_last=True)
        assert not max(_sliced_ratios(n, m, l, res, bad, dirs)) <= 10.0, (entry, "last")
        if m % n:
            bad = SL.sliced_one(c.x[0], c.y[0], dirs, rsw=SL.pairs_by_formula(n, m, floor_defect=True))
            assert not max(_sliced_ratios(n, m, l, res, bad, dirs)) <= 10.0, (entry, "floor")
    if family in ("plane", "line", "collapsed", "duplicates", "offset_1000"):
        bad = SL.sliced_one(c.x[0], c.y[0], dirs, order_flags={"descending_ties": True})
        assert not np.array_equal(res["order1"], bad["order1"]), (entry, "ties")


def _dcd_ratios(res, other, alpha, lam, n, m):
    bl, bc, b1, b2 = D.bounds(res, alpha, lam, n, m)
    out = []
    for key, bound in (("loss", bl), ("cd", bc), ("gd1", b1), ("gd2", b2)):
        err = np.abs(np.asarray(other[key], np.float64) - res[key])
        out.append(float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)))))
    return out


@pytest.mark.parametrize("entry", G.entries("dcd"), ids=_ids("dcd"))
def test_dcd_float32_restatement_and_defects(oracle, entry):
    """The float32 evaluation inside dcd_restated.bounds on every case and lambda; each modelled defect that
    the case exercises leaves them by more than ten bounds."""
    family, shape = entry
    c = G.case("dcd", family, shape)
    n, m = c.x.shape[1], c.y.shape[1]
    d1, d2, i1, i2, alpha = G.dcd_forward(family, shape)
    for lam in G.DCD_LAMBDAS:
        res = G.dcd_reference(family, shape, lam)
        f32 = D.evaluate(d1, d2, i1, i2, alpha, lam, False, dtype=np.float32)
        figures = _dcd_ratios(res, f32, alpha, lam, n, m)
        assert max(figures) <= 1.0, (entry, lam, figures)
        defects = ["cross_counts", "drop_tail"] + (["swap_r"] if n != m else []) + (["ignore_lambda"] if lam == 0.5 else [])
        if family == "identical":  # every count is 1: the histograms agree and a power of 1 is 1
            defects = ["drop_tail"]
        for defect in defects:
            bad = D.evaluate(d1, d2, i1, i2, alpha, lam, False, defect=defect)
            figures = _dcd_ratios(res, bad, alpha, lam, n, m)
            assert max(figures[0], figures[2], figures[3]) > 10.0, (entry, lam, defect, figures)


@pytest.mark.parametrize("kernel", K.KERNELS, ids=K.KERNEL_NAMES.get)
def test_kernel_loss_cases_show_a_dropped_tile_or_block(kernel):
    """As test_kernel_loss_cpu.py demands of its inputs, on every case: the first tile of columns left out of
    every row sum, or the first block of rows left out, moves the float64 result by more than ten bounds -- the
    loss by ten loss bounds or, where the loss hides it, a gradient component by ten gradient bounds (a left-out
    block of rows leaves its points' gradients unwritten; left-out columns are missing from every point's sum).
    The gradient is needed for `line` (rows of x move the Gaussian loss by 9.1 bounds at (257, 255)) and for
    identical clouds, where the own and the cross sums lose the same terms and the loss stays 0.  With identical
    clouds a row's loss term and gradient are 0 whatever the kernel: only the columns can show there."""
    for family, shape in G.entries("kernel"):
        c = G.case("kernel", family, shape)
        n, m = c.x.shape[1], c.y.shape[1]
        blur = G.KERNEL_BLUR * c.s
        bound = K.loss_bound(kernel, n, m, K.diameter(c.x, c.y))
        bx, by = K.grad_bound(kernel, n, m, blur)
        for bi in range(shape[0]):
            mats = K.pair_matrices(c.x[bi], c.y[bi], kernel, blur)
            full = K.loss_from(mats)
            gx, gy = K.grads_from(mats, kernel, blur)
            want = K.restated_one(c.x[bi], c.y[bi], kernel, blur)
            # the one formula, to the double sums' order (p sum g - g q cancels eleven digits at coordinate 1000)
            for g, w in ((gx, want[1]), (gy, want[2])):
                assert np.abs(g - w).max() <= 1e-3 * min(bx, by)
            for cloud, cnt in ((0, n), (1, m)):
                keep = [np.ones(n, bool), np.ones(m, bool)]
                keep[cloud][:min(K.TILE, cnt)] = False
                hx, hy = K.grads_from(mats, kernel, blur, keep)
                moved = max(abs(K.loss_from(mats, skip_cols=(cloud, 0, min(K.TILE, cnt))) - full) / bound,
                            np.abs(hx - gx).max() / bx, np.abs(hy - gy).max() / by)
                assert moved > 10, (family, shape, "columns", cloud, moved)
                if family != "identical":
                    rows = slice(0, min(K.ROWS, cnt))
                    moved = max(abs(K.loss_from(mats, skip_rows=(cloud, 0, min(K.ROWS, cnt))) - full) / bound,
                                np.abs((gx, gy)[cloud][rows]).max() / (bx, by)[cloud])
                    assert moved > 10, (family, shape, "rows", cloud, moved)


# ---------------------------------------------------------------------------
# power-of-two scaling keeps bits
# ---------------------------------------------------------------------------
def test_scaling_by_1024_keeps_seeds_lists_and_orders():
    for shape in G.SHAPES["fps"]:
        assert np.array_equal(G.fps_reference("scale_1024", shape), G.fps_reference("unit", shape))
    (d0, i0), (d1, i1) = G.knn_reference("unit"), G.knn_reference("scale_1024")
    assert np.array_equal(i0, i1) and np.array_equal((d0 * np.float32(2.0 ** 20)).view(np.int32), d1.view(np.int32))
    for shape in G.SHAPES["sliced"]:
        a, b = G.sliced_reference("unit", shape)[1], G.sliced_reference("scale_1024", shape)[1]
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["order1"], rb["order1"]) and np.array_equal(ra["order2"], rb["order2"])
    for r in range(len(G.BALL_RADII)):
        a, b = G.ball_reference("unit", r), G.ball_reference("scale_1024", r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
