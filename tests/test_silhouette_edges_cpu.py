"""tests/silhouette_restated.py checked without a GPU: the cases meet the
launch-geometry edges of csrc/silhouette.hip they are there for, and at every
case the float32 restatement of the forward, the backward and the BCE loss
stays within a quarter of the tolerance tests/test_silhouette_edges_gpu.py and
tests/test_silhouette_gpu.py hold the device to -- so the tolerance leaves room
for the kernels' own order of summation and the hardware exponential, and a
restatement that drops a row, a column, a point or a partial leaves it."""
import os
import re

import numpy as np
import pytest

import silhouette_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pcm.h")
_worst = {}


def _chain():
    return int(re.search(r"#define\s+PCM_PROJ_BCE_CHAIN\s+(\d+)", open(HEADER).read()).group(1))


def _ratio(err, bound):
    return float(np.max(np.where(err == 0, 0.0, err / bound), initial=0.0))


def test_the_cases_meet_the_launch_geometry_edges():
    assert R.B == 3 and len(R.FAMILIES) == 6
    assert all(1 <= v <= 128 for g in R.BWD_GRIDS for v in g)
    # forward: one row, one column, a partial tile after 1, 2 and 3 full ones in either direction
    for axis in (0, 1):
        sizes = {g[axis] for g in R.FWD_GRIDS}
        assert {1, 33, 65, 127, 128} <= sizes
        assert {v // 32 for v in sizes if v % 32} == {0, 1, 2, 3}  # full tiles before the partial one
    assert {n % 128 for n in R.FWD_COUNTS} >= {15, 16, 17, 127, 0, 1}
    # backward: every slice count with a partial band of rows after a full one, and widths just past an edge
    # (one slice, widths up to 8, meets it at the point-count cases' grid (33, 8))
    assert {R.bwd_slices(w)[0] for h, w in R.BWD_GRIDS if h > 32 and h % 32} == {2, 4, 8, 16}
    assert {R.bwd_slices(c.grid[1])[0] for c in R.BWD_CASES if c.grid[0] > 32 and c.grid[0] % 32} == {1, 2, 4, 8, 16}
    assert {9, 17, 33, 65} <= {w for _, w in R.BWD_GRIDS}
    for w, p in R.BWD_POINTS.items():
        assert R.bwd_slices(w)[1] == p
        assert {c.n for c in R.BWD_CASES if c.grid == (R.BWD_COUNT_HEIGHT, w)} >= {p - 1, p, p + 1}
    for cases in (R.FWD_CASES, R.BWD_CASES):
        assert len(set(cases)) == len(cases)
        for g in R.SIGMA_GRIDS:
            assert {(c.family, c.sigma_sq) for c in cases if c.grid == g and c.n == R.N} == {
                (f, s) for f in R.FAMILIES for s in R.SIGMAS}
        assert all(c.sigma_sq == 0.5 for c in cases if c.grid not in R.SIGMA_GRIDS)
    assert R.BCE_NEW_COUNTS == (2047, 2048, 2049, 524288, 524289, 526336, 1048576)


def test_the_input_families_do_what_they_claim():
    for grid in ((33, 31), (100, 9), (128, 127), (1, 1), (8, 17)):
        h, w = grid
        for family in R.FAMILIES:
            xyz = R.cloud(family, grid, R.N)
            assert xyz.shape == (R.B, R.N, 3) and xyz.dtype == np.float32
            assert np.isfinite(xyz[..., :2]).all() and np.isnan(xyz[:, ::3, 2]).all()
            assert np.isfinite(xyz[:, 1::3, 2]).all()
        gx, gy = R._pinned(R.cloud("wide", grid, R.N), h, w)
        assert gx.min() < -0.5 * h and gx.max() > 1.5 * h - 1
        gx, gy = R._pinned(R.cloud("centres", grid, R.N), h, w)
        k = np.arange(R.N)
        # the float32 map cannot reach every integer (81 of 100 rows, 7 of 9 columns at (100, 9)); the rest
        # sit a few 1e-6 off their cell
        on_x, on_y = gx == (k % h), gy == ((k // h) % w)
        print(grid, "points exactly on their row:", int(on_x.sum()), "column:", int(on_y.sum()), "of", on_x.size)
        assert on_x.mean() >= 0.5 and on_y.mean() >= 0.3 and (on_x & on_y).any()
        assert np.abs(gx - k % h).max() < 1e-5 and np.abs(gy - (k // h) % w).max() < 1e-5
        gx, _ = R._pinned(R.cloud("edge", grid, R.N), h, w)
        assert (gx[:, 0::2] == 0).all() and (gx[:, 1::2] == h).all()  # (p + 1) rounds to 2 from just below 1
        xyz = R.cloud("duplicates", grid, R.N)
        assert np.array_equal(xyz[:, R.N // 2:, :2], xyz[:, :R.N // 2, :2])
        xyz = R.cloud("collapsed", grid, R.N)
        assert (xyz[..., 0] == np.float32(0.3)).all() and (xyz[..., 1] == np.float32(-0.6)).all()
    # `wide` leaves whole tiles 0 at the narrow kernel and 0.02 a cell 0 between two points' cells
    assert (R.sil_f64(R.cloud("wide", (128, 127), R.N), 128, 127, 0.02) == 0).mean() > 0.5


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_forward_float32_restatement_within_a_quarter(case):
    h, w = case.grid
    xyz = R.cloud(case.family, case.grid, case.n)
    want = R.sil_f64(xyz, h, w, case.sigma_sq)
    got = R.sil_f32(xyz, h, w, case.sigma_sq).astype(np.float64)
    assert np.isfinite(want).all() and want.shape == (R.B, h, w)
    ratio = _ratio(np.abs(got - want), R.FWD_RTOL * np.abs(want) + R.FWD_ATOL)
    key = ("forward", case.grid, case.sigma_sq)
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    assert ratio <= 0.25, (case, ratio)


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.case_id)
def test_backward_float32_restatement_within_a_quarter(case):
    h, w = case.grid
    xyz = R.cloud(case.family, case.grid, case.n)
    G = R.grad_sil(case.grid, case.n)
    want, A = R.grad_f64(xyz, G, h, w, case.sigma_sq)
    got = R.grad_f32(xyz, G, h, w, case.sigma_sq).astype(np.float64)
    assert np.isfinite(want).all() and not got[..., 2].any()
    ratio = _ratio(np.abs(got[..., :2] - want[..., :2]), R.backward_bound(h, w, A))
    key = ("backward", case.grid, case.sigma_sq)
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    assert ratio <= 0.25, (case, ratio)


@pytest.mark.parametrize("w", [1.0, 0.5])
@pytest.mark.parametrize("count", R.BCE_COUNTS + R.BCE_NEW_COUNTS)
def test_bce_float32_restatement_within_a_quarter(count, w):
    L = _chain()
    for gt_scale in R.BCE_GT_SCALES:
        pred, gt = R.bce_inputs(count, gt_scale)
        term, _ = R._bce_f64(pred.numpy(), gt.numpy(), w)
        want = term.sum() / float(np.float32(count))
        got = float(R.bce_loss_f32(R.bce_terms_f32(pred.numpy(), gt.numpy(), w)))
        ratio = abs(got - want) / R.bce_tolerance(term, L)
        key = ("bce", count, gt_scale)
        _worst[key] = max(_worst.get(key, 0.0), ratio)
        assert ratio <= 0.25, (count, w, gt_scale, ratio)


@pytest.mark.parametrize("w", [1.0, 0.5])
def test_bce_edge_vector_float32_restatement_within_a_quarter(w):
    L = _chain()
    preds, gts = R.bce_edge_vector()
    term, grad = R._bce_f64(preds, gts, w)
    assert np.isfinite(term).all() and np.isfinite(grad).all()
    t32 = R.bce_terms_f32(preds, gts, w).astype(np.float64)
    # per element, as the device is checked: count = 1, mean|term| = |term|
    per = np.abs(t32 - term) / ((L + 8) * R.U * np.abs(term) + 2.4e-7)
    print("edge vector w", w, "per element worst", per.max())
    assert per.max() <= 0.25
    # and summed: the log(1e-8) terms (|term| up to 37) stay in -- the quarter holds with them
    got = float(R.bce_loss_f32(R.bce_terms_f32(preds, gts, w)))
    ratio = abs(got - term.sum() / float(np.float32(preds.size))) / R.bce_tolerance(term, L)
    print("edge vector w", w, "summed", ratio)
    assert ratio <= 0.25


def test_record_worst_ratio():
    """After the comparisons above (same process): the worst float32 error over a quarter-checked tolerance."""
    for kind in ("forward", "backward", "bce"):
        vals = {k: v for k, v in _worst.items() if k[0] == kind}
        if vals:
            k = max(vals, key=vals.get)
            print(kind, "worst error / tolerance", f"{vals[k]:.3g}", "at", k[1:])
