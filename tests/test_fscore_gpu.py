"""GPU checks of the one-pass Chamfer evaluation (csrc/chamfer_eval.hip) and its
callers: pcm_hip.chamfer_eval, chamfer_3DEval, loss_.fscore and the F-Score
item of Metrics.

References: the committed fixture generated from the reference's own
loss/loss_.py (tests/golden/make_fscore_golden.py), the CPU oracle's pinned
distances, and chamfer_3DDist on the same device.  Counts are compared
exactly; values that the reference forms with one or two roundings more
(torch's mean as sum * fl(1/N) where the library divides) within rtol 1e-6
(about 8 ulp), and mean distances within the project's documented rtol 1e-5
of the float64 mean: the terms are non-negative, so the relative error of a
float32 sum is at most (longest sequential chain) * 2^-24, and the kernel's
chains are 6 DPP steps, 8 waves and one term per workgroup of a cloud (at
most 40 at the shapes below).
"""
import functools
import os

import numpy as np
import pytest
import torch

from fscore_restated import batch_from as _batch_from
from fscore_restated import bits as _bits
from fscore_restated import counts_from as _counts_from
from fscore_restated import scores_from as _scores_from

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fscore_golden.npz")
THS = (1e-4, 1e-3, 1e-2, 1.0, 30.0)


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _golden_cases():
    return [str(c) for c in _golden()["cases"]]


def _run(cuda, a, c, ths, workspace=None, with_batch=True):
    """pcm_hip.chamfer_eval on host clouds (float32 or float16 tensors) ->
    numpy (mean_dist [B,2], counts [B,T,2], scores [B,T,3], batch [T,3])."""
    import pcm_hip
    x1, x2 = a.to(cuda).contiguous(), c.to(cuda).contiguous()
    b, t = x1.shape[0], len(ths)
    md = torch.full((b, 2), -7.0, device=cuda)
    cn = torch.full((b, t, 2), -7, dtype=torch.int32, device=cuda)
    sc = torch.full((b, t, 3), -7.0, device=cuda)
    bs = torch.full((t, 3), -7.0, device=cuda) if with_batch else None
    pcm_hip.chamfer_eval(x1, x2, ths, md, cn, sc, bs, workspace=workspace)
    torch.cuda.synchronize()
    return (md.cpu().numpy(), cn.cpu().numpy(), sc.cpu().numpy(), bs.cpu().numpy() if with_batch else None)


# ---- reference parity ---------------------------------------------------------

@pytest.mark.parametrize("case", _golden_cases())
def test_reference_parity_on_the_fixture(cuda, case):
    z = _golden()
    ths = tuple(float(t) for t in z["thresholds"])
    a, c = torch.from_numpy(z[f"{case}/xyz1"]), torch.from_numpy(z[f"{case}/xyz2"])
    md, cn, sc, bs = _run(cuda, a, c, ths)
    np.testing.assert_array_equal(cn[:, :, 0], z[f"{case}/count_x"])
    np.testing.assert_array_equal(cn[:, :, 1], z[f"{case}/count_y"])
    # the reference's triple is (fscore, precision_1 = share of Y, precision_2 = share of X)
    ref = z[f"{case}/per_cloud"]
    print(case, "per-cloud max rel err",
          [float(np.max(np.abs(sc[:, :, k] - ref[:, :, j]) / np.maximum(np.abs(ref[:, :, j]), 1e-30)))
           for k, j in ((0, 0), (2, 1), (1, 2))])
    np.testing.assert_allclose(sc[:, :, 0], ref[:, :, 0], rtol=1e-6, atol=0)
    np.testing.assert_allclose(sc[:, :, 2], ref[:, :, 1], rtol=1e-6, atol=0)
    np.testing.assert_allclose(sc[:, :, 1], ref[:, :, 2], rtol=1e-6, atol=0)
    refb = z[f"{case}/batch"]
    np.testing.assert_allclose(bs[:, 0], refb[:, 0], rtol=1e-6, atol=0)
    np.testing.assert_allclose(bs[:, 2], refb[:, 1], rtol=1e-6, atol=0)
    np.testing.assert_allclose(bs[:, 1], refb[:, 2], rtol=1e-6, atol=0)


# ---- oracle and product parity ------------------------------------------------

# (b, n, m): single points; tiny ragged; under one wave; across the 2048-point
# LDS tile; config 2's cloud; config 2; ragged multi-block; the two sides
# of the 2- / 4-queries-per-lane switch (512 workgroups of 256 queries); and
# exactly one and exactly two LDS tiles (no padded chunk, no partial tile)
SHAPES = [(1, 1, 1), (2, 5, 3), (2, 33, 31), (1, 2049, 2047), (3, 1024, 1024), (32, 1024, 1024), (2, 5000, 700),
          (255, 70, 50), (256, 70, 50), (64, 1030, 700), (1, 2048, 2048), (1, 4096, 2048)]


@functools.lru_cache(maxsize=None)
def _shape_case(shape):
    """Clouds of a shape and the oracle's forward on them, computed once."""
    import oracle as O
    O.build()
    b, n, m = shape
    g = torch.Generator().manual_seed(1000 + b * 7 + n * 3 + m)
    if shape == (2, 5, 3):
        a, c = torch.randn(b, n, 3, generator=g) * 10, torch.randn(b, m, 3, generator=g) * 10
    else:
        a, c = torch.rand(b, n, 3, generator=g), torch.rand(b, m, 3, generator=g)
    d1, d2, _, _ = O.chamfer_forward(a.numpy(), c.numpy())
    return a, c, d1, d2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_and_product_parity(cuda, oracle, shape):
    import dist_chamfer_3D
    b, n, m = shape
    a, c, d1, d2 = _shape_case(shape)
    md, cn, sc, bs = _run(cuda, a, c, THS)
    # counts: the oracle's distances, and chamfer_3DDist's on this device
    np.testing.assert_array_equal(cn[:, :, 0], _counts_from(d1, THS))
    np.testing.assert_array_equal(cn[:, :, 1], _counts_from(d2, THS))
    g1, g2, _, _ = dist_chamfer_3D.chamfer_3DDist()(a.to(cuda), c.to(cuda))
    np.testing.assert_array_equal(cn[:, :, 0], _counts_from(g1.cpu().numpy(), THS))
    np.testing.assert_array_equal(cn[:, :, 1], _counts_from(g2.cpu().numpy(), THS))
    # mean distances against the float64 mean of the oracle's distances
    ref = np.stack([d1.astype(np.float64).mean(1), d2.astype(np.float64).mean(1)], 1)
    print(shape, "mean_dist max rel err", float(np.max(np.abs(md - ref) / ref)))
    np.testing.assert_allclose(md, ref, rtol=1e-5, atol=0)
    # scores and batch means: the pinned arithmetic on those counts, bit for bit
    want = _scores_from(cn[:, :, 0], cn[:, :, 1], n, m)
    np.testing.assert_array_equal(_bits(sc), _bits(want))
    np.testing.assert_array_equal(_bits(bs), _bits(_batch_from(want)))


def test_module_returns_the_named_tuple(cuda):
    import eval_chamfer_3D
    a, c, d1, d2 = _shape_case((2, 33, 31))
    out = eval_chamfer_3D.chamfer_3DEval(THS)(a.to(cuda).requires_grad_(True), c.to(cuda))
    md, cn, sc, _ = _run(cuda, a, c, THS)
    assert out._fields == ("mean_dist1", "mean_dist2", "count1", "count2", "precision", "recall", "fscore")
    assert all(t.device.type == "cuda" and not t.requires_grad for t in out)
    assert out.count1.dtype == torch.int32 and out.count2.dtype == torch.int32
    assert tuple(out.mean_dist1.shape) == (2,) and tuple(out.fscore.shape) == (2, len(THS))
    np.testing.assert_array_equal(_bits(out.mean_dist1.cpu().numpy()), _bits(md[:, 0]))
    np.testing.assert_array_equal(_bits(out.mean_dist2.cpu().numpy()), _bits(md[:, 1]))
    np.testing.assert_array_equal(out.count1.cpu().numpy(), cn[:, :, 0])
    np.testing.assert_array_equal(out.count2.cpu().numpy(), cn[:, :, 1])
    np.testing.assert_array_equal(_bits(out.fscore.cpu().numpy()), _bits(sc[:, :, 0]))
    np.testing.assert_array_equal(_bits(out.precision.cpu().numpy()), _bits(sc[:, :, 1]))
    np.testing.assert_array_equal(_bits(out.recall.cpu().numpy()), _bits(sc[:, :, 2]))
    # a transposed view is made contiguous rows
    planes = a.transpose(1, 2).contiguous().to(cuda)
    out2 = eval_chamfer_3D.chamfer_3DEval(THS)(planes.transpose(1, 2), c.to(cuda))
    assert torch.equal(out2.count1, out.count1) and torch.equal(out2.fscore, out.fscore)


# ---- threshold edges -----------------------------------------------------------

def _lattice():
    """All 512 points k/8, k in 0..7, and the same shifted by 1/8 along x:
    every distance is an exact multiple of 1/64.  448 points of either cloud
    coincide with a point of the other; 64 are exactly 1/64 away."""
    k = torch.arange(8, dtype=torch.float32) / 8
    a = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), -1).reshape(1, 512, 3)
    c = a + torch.tensor([0.125, 0.0, 0.0])
    return a, c


def test_threshold_equal_to_an_attained_distance_is_strict(cuda):
    a, c = _lattice()
    just_above = float(np.nextafter(np.float32(1 / 64), np.float32(1)))
    md, cn, sc, bs = _run(cuda, a, c, (1 / 64, just_above))
    np.testing.assert_array_equal(cn[0, 0], [448, 448])  # the 64 points at exactly 1/64 are not counted
    np.testing.assert_array_equal(cn[0, 1], [512, 512])
    np.testing.assert_array_equal(md[0], np.float32([64 * (1 / 64) / 512] * 2))  # exact sums


def test_threshold_zero_and_infinity(cuda):
    a, c = _lattice()
    md, cn, sc, bs = _run(cuda, a[:, :300], c[:, :200], (0.0, float("inf")))
    np.testing.assert_array_equal(cn[0, 0], [0, 0])
    np.testing.assert_array_equal(sc[0, 0], [0.0, 0.0, 0.0])  # f == 0, not NaN
    np.testing.assert_array_equal(bs[0], [0.0, 0.0, 0.0])
    np.testing.assert_array_equal(cn[0, 1], [300, 200])
    np.testing.assert_array_equal(sc[0, 1], [1.0, 1.0, 1.0])
    assert np.isfinite(sc).all() and np.isfinite(bs).all()


def test_identical_clouds_score_one(cuda):
    a, _, _, _ = _shape_case((2, 33, 31))
    md, cn, sc, bs = _run(cuda, a, a.clone(), (1e-4,))
    np.testing.assert_array_equal(cn[:, 0], [[33, 33], [33, 33]])
    np.testing.assert_array_equal(sc[:, 0], [[1.0, 1.0, 1.0]] * 2)
    np.testing.assert_array_equal(bs[0], [1.0, 1.0, 1.0])
    np.testing.assert_array_equal(md, np.zeros((2, 2), np.float32))


def test_eight_unsorted_thresholds_equal_eight_single_calls(cuda):
    g = torch.Generator().manual_seed(11)
    a, c = torch.rand(2, 300, 3, generator=g), torch.rand(2, 200, 3, generator=g)
    ths = (3e-3, 1e-4, 0.5, 1e-2, 2.5e-4, 0.0, 1e-3, 5e-2)
    md, cn, sc, bs = _run(cuda, a, c, ths)
    assert len(np.unique(cn[:, :, 0].sum(0))) > 4  # the thresholds do separate the points
    for t, th in enumerate(ths):
        md1, cn1, sc1, bs1 = _run(cuda, a, c, (th,))
        np.testing.assert_array_equal(cn1[:, 0], cn[:, t])
        np.testing.assert_array_equal(_bits(sc1[:, 0]), _bits(sc[:, t]))
        np.testing.assert_array_equal(_bits(bs1[0]), _bits(bs[t]))
        np.testing.assert_array_equal(_bits(md1), _bits(md))


# ---- non-finite coordinates ---------------------------------------------------

@pytest.mark.parametrize("nan_at,inf_at", [((1, 2048, 0), (0, 700, 2)), ((0, 1300, 1), (1, 512, 0))],
                         ids=["nan_tile_start_inf_mid", "nan_mid_inf_tile_start"])
def test_non_finite_counts_follow_the_forward(cuda, nan_at, inf_at):
    # (cloud 0 = xyz1 / 1 = xyz2, point, coordinate), all in batch element 0;
    # batch element 1 stays finite
    import dist_chamfer_3D
    g = torch.Generator().manual_seed(21)
    clouds = [torch.rand(2, 2100, 3, generator=g), torch.rand(2, 2100, 3, generator=g)]
    clouds[nan_at[0]][0, nan_at[1], nan_at[2]] = float("nan")
    clouds[inf_at[0]][0, inf_at[1], inf_at[2]] = float("inf")
    a, c = clouds
    ths = (1e-4, 1e-3, 1e-2, float("inf"))
    md, cn, sc, bs = _run(cuda, a, c, ths)
    d1, d2, _, _ = dist_chamfer_3D.chamfer_3DDist()(a.to(cuda), c.to(cuda))
    np.testing.assert_array_equal(cn[:, :, 0], _counts_from(d1.cpu().numpy(), ths))
    np.testing.assert_array_equal(cn[:, :, 1], _counts_from(d2.cpu().numpy(), ths))
    # the finite element's means are unaffected
    ref = np.stack([d1[1].double().mean().item(), d2[1].double().mean().item()])
    np.testing.assert_allclose(md[1], ref, rtol=1e-5, atol=0)


# ---- fp16 ---------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 300, 200), (1, 4096, 4096)], ids=lambda s: "x".join(map(str, s)))
def test_fp16_equals_fp32_on_widened_clouds(cuda, shape):
    b, n, m = shape
    g = torch.Generator().manual_seed(31)
    a, c = torch.rand(b, n, 3, generator=g).half(), torch.rand(b, m, 3, generator=g).half()
    half = _run(cuda, a, c, THS)
    wide = _run(cuda, a.float(), c.float(), THS)
    assert half[1][:, 2].sum() > 0  # fp16 clouds are coarse, but the counts are not trivially empty
    for h, w in zip(half, wide):
        np.testing.assert_array_equal(_bits(h), _bits(w))


def test_fp16_non_finite_equals_fp32_on_widened_clouds(cuda):
    # a NaN at a tile start of xyz2 and a +inf in mid-cloud of xyz1, both in batch element 0: its workgroups
    # divert to the reference-exact scan in either entry; batch element 1 stays finite
    g = torch.Generator().manual_seed(33)
    a, c = torch.rand(2, 2100, 3, generator=g).half(), torch.rand(2, 2100, 3, generator=g).half()
    c[0, 2048, 0] = float("nan")
    a[0, 700, 2] = float("inf")
    assert torch.isfinite(a[1]).all() and torch.isfinite(c[1]).all()
    ths = (1e-4, 1e-3, 1e-2, float("inf"))
    half = _run(cuda, a, c, ths)
    wide = _run(cuda, a.float(), c.float(), ths)
    assert 0 < half[1][1, 2].sum() and half[1][1, 3].tolist() == [2100, 2100]
    assert half[1][0, 3].sum() < 4200  # the non-finite points do reach the counts of element 0
    assert np.isfinite(half[0][1]).all()
    for h, w in zip(half, wide):
        np.testing.assert_array_equal(_bits(h), _bits(w))


# ---- determinism, workspace, streams, graphs ------------------------------------

def test_deterministic_and_workspace_content_is_irrelevant(cuda):
    import pcm_hip
    a, c, _, _ = _shape_case((3, 1024, 1024))
    first = _run(cuda, a, c, THS)
    second = _run(cuda, a, c, THS)
    need = pcm_hip.load_library().pcm_chamfer_eval_workspace_bytes(3, 1024, 1024, len(THS))
    junk = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    third = _run(cuda, a, c, THS, workspace=junk)
    nob = _run(cuda, a, c, THS, with_batch=False)
    for k in range(4):
        np.testing.assert_array_equal(_bits(first[k]), _bits(second[k]))
        np.testing.assert_array_equal(_bits(first[k]), _bits(third[k]))
    for k in range(3):  # batch_scores is optional
        np.testing.assert_array_equal(_bits(first[k]), _bits(nob[k]))
    with pytest.raises(pcm_hip.PcmError):
        _run(cuda, a, c, THS, workspace=junk[:64])


def test_side_stream_and_graph_replay(cuda):
    import pcm_hip
    a, c, _, _ = _shape_case((3, 1024, 1024))
    want = _run(cuda, a, c, THS)
    x1, x2 = a.to(cuda), c.to(cuda)
    t = len(THS)

    def outputs():
        return (torch.empty(3, 2, device=cuda), torch.empty(3, t, 2, dtype=torch.int32, device=cuda),
                torch.empty(3, t, 3, device=cuda), torch.empty(t, 3, device=cuda))

    side = outputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pcm_hip.chamfer_eval(x1, x2, THS, *side)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for got, w in zip(side, want):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(w))

    # one capture, replayed after the input buffers are overwritten in place
    cap = outputs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm_hip.chamfer_eval(x1, x2, THS, *cap)
    g = torch.Generator().manual_seed(41)
    a2, c2 = torch.rand(3, 1024, 3, generator=g), torch.rand(3, 1024, 3, generator=g)
    x1.copy_(a2)
    x2.copy_(c2)
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(cuda, a2, c2, THS)
    assert not np.array_equal(eager[1], want[1])
    for got, w in zip(cap, eager):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(w))


# ---- callers ---------------------------------------------------------------------

def test_loss_module_functions(cuda, oracle):
    import loss_
    z = _golden()
    case = "noisy_ragged"
    a, c = torch.from_numpy(z[f"{case}/xyz1"]), torch.from_numpy(z[f"{case}/xyz2"])
    x, y = a.to(cuda), c.to(cuda)
    for t, th in enumerate(z["thresholds"]):
        f, p1, p2 = loss_.fscore(x, y, float(th))
        for v in (f, p1, p2):
            assert v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda"
        assert f.requires_grad and not p1.requires_grad
        np.testing.assert_allclose([f.item(), p1.item(), p2.item()], z[f"{case}/batch"][t], rtol=1e-6, atol=0)
    f_default = loss_.fscore(x, y)[0]
    assert f_default.item() == loss_.fscore(x, y, 0.0001)[0].item()
    r1, r2, j1, j2 = oracle.chamfer_forward(a.numpy(), c.numpy())
    total, mins1, mins2 = loss_.batch_NN_loss(x, y)
    np.testing.assert_array_equal(_bits(mins1.cpu().numpy()), _bits(r2))  # per-y-point
    np.testing.assert_array_equal(_bits(mins2.cpu().numpy()), _bits(r1))  # per-x-point
    ref_total = r1.astype(np.float64).mean() + r2.astype(np.float64).mean()
    assert abs(total.item() - ref_total) <= 1e-5 * ref_total
    assert abs(loss_.cd(x, y).item() - ref_total) <= 1e-5 * ref_total
    d1, d2, i1, i2 = loss_.distChamfer(x, y)
    assert i1.dtype == torch.int32 and i2.dtype == torch.int32
    np.testing.assert_array_equal(i1.cpu().numpy(), j1)
    np.testing.assert_array_equal(i2.cpu().numpy(), j2)
    np.testing.assert_array_equal(_bits(d1.cpu().numpy()), _bits(r1))


def test_metrics_fscore_item(cuda):
    import loss_
    import metrics
    z = _golden()
    a = torch.from_numpy(z["noisy_1024/xyz1"]).to(cuda)
    c = torch.from_numpy(z["noisy_1024/xyz2"]).to(cuda)
    item = metrics.Metrics.ITEMS[2]
    assert item["name"] == "F-Score" and item["enabled"] is False
    base = metrics.Metrics.get(a, c)
    assert len(base) == 2
    item["enabled"] = True
    try:
        assert metrics.Metrics.names() == ["EMD_distance", "ChamferDistance", "F-Score"]
        vals = metrics.Metrics.get(a, c)
    finally:
        item["enabled"] = False
    assert len(vals) == 3 and vals[:2] == base
    assert isinstance(vals[2], float) and 0.0 <= vals[2] <= 1.0
    assert vals[2] == loss_.fscore(a, c, metrics.EVAL_FSCORE_THRESHOLD)[0].item()
    np.testing.assert_allclose(vals[2], z["noisy_1024/batch"][0, 0], rtol=1e-6, atol=0)
    assert metrics.Metrics.names() == ["EMD_distance", "ChamferDistance"]
