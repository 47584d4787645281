"""pcm_chamfer_nd_forward / pcm_chamfer_nd_backward (csrc/chamfer_nd.hip) on the
device against the contract restated in numpy (tests/chamfer_nd_restated.py).

The rule is bit equality: distances and gradients compared as int32 bits,
indices equal, every output prefilled with a sentinel the call must overwrite.
Sizes are the smallest that reach each seam of the kernels: T candidates a
tile, QB queries a workgroup, W waves that share a tile."""
import os
import sys

import numpy as np
import pytest
import torch

import chamfer_nd_restated as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND_DIR = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "metric", "chamferND")
if ND_DIR not in sys.path:
    sys.path.insert(0, ND_DIR)

import pcm_hip  # noqa: E402
import dist_chamfer_ND as ND  # noqa: E402

pytestmark = pytest.mark.gpu

T, QB, W = pcm_hip.CHAMFER_ND_TILE, pcm_hip.CHAMFER_ND_QUERIES, pcm_hip.CHAMFER_ND_WAVES
# (n, m): n from {1, QB - 1, QB, QB + 1, 2 QB + 5}, m from {1, 63, 65, T/W - 1, T/W + 1, T - 1, T, T + 1, 2 T + 3},
# every value at least once, n != m throughout so that a swapped direction cannot pass
PAIRS = [(1, 63), (QB - 1, 1), (QB, 65), (QB + 1, T // W - 1), (2 * QB + 5, T // W + 1), (1, T - 1), (QB - 1, T),
         (QB, T + 1), (QB + 1, 2 * T + 3)]
NAN, INF = float("nan"), float("inf")


def _planes(t):
    """The same cloud as a [B, N, D] view of contiguous channel planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _dev(x, cuda, planes=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    return _planes(t) if planes else t


def _forward(x1, x2, lay1=0, lay2=0):
    """The raw entry on device clouds, outputs prefilled with sentinels -> numpy."""
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    dev = x1.device
    d1 = torch.full((b, n), -1.0, device=dev)
    d2 = torch.full((b, m), -1.0, device=dev)
    i1 = torch.full((b, n), -7, dtype=torch.int32, device=dev)
    i2 = torch.full((b, m), -7, dtype=torch.int32, device=dev)
    pcm_hip.chamfer_nd_forward(x1, lay1, x2, lay2, d1, d2, i1, i2)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (d1, d2, i1, i2))


def _backward(x1, x2, gd1, gd2, i1, i2, lay1=0, lay2=0):
    dev = x1.device
    g1 = torch.full(x1.shape, NAN, device=dev)
    g2 = torch.full(x2.shape, NAN, device=dev)
    if lay1:
        g1 = _planes(g1)
    if lay2:
        g2 = _planes(g2)
    as_t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)  # noqa: E731
    pcm_hip.chamfer_nd_backward(x1, lay1, x2, lay2, as_t(gd1, torch.float32), as_t(gd2, torch.float32),
                                as_t(i1, torch.int32), as_t(i2, torch.int32), g1, g2)
    torch.cuda.synchronize()
    return g1.cpu().numpy(), g2.cpu().numpy()


def _same_forward(got, want, what=""):
    for g, w, name in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        if name.startswith("dist"):
            np.testing.assert_array_equal(R.bits(g), R.bits(w), err_msg=f"{name} {what}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{name} {what}")


def _same_bits(got, want, what=""):
    np.testing.assert_array_equal(R.bits(got), R.bits(want), err_msg=what)


# ---- 1. values -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", range(1, 9))
def test_values_at_every_seam(cuda, dim):
    for n, m in PAIRS:
        x1, x2 = R.make_clouds(1000 * dim + n + m, 2, n, m, dim)
        _same_forward(_forward(_dev(x1, cuda), _dev(x2, cuda)), R.forward_restated(x1, x2), f"D={dim} n={n} m={m}")


# ---- 2. D = 3 against the product ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m", [(65, 300), (1030, 257)])
def test_dim3_equals_chamfer_3d(cuda, n, m):
    from dist_chamfer_3D import chamfer_3DDist
    x1, x2 = R.make_clouds(n, 2, n, m, 3)
    rng = np.random.default_rng(m)
    gd1 = torch.from_numpy(rng.standard_normal((2, n)).astype(np.float32)).to(cuda)
    gd2 = torch.from_numpy(rng.standard_normal((2, m)).astype(np.float32)).to(cuda)
    outs = []
    for dist in (ND.chamfer_NDDist(), chamfer_3DDist()):
        a, c = _dev(x1, cuda).requires_grad_(), _dev(x2, cuda).requires_grad_()
        d1, d2, i1, i2 = dist(a, c)
        torch.autograd.backward([d1, d2], [gd1, gd2])
        outs.append([t.detach().cpu().numpy() for t in (d1, d2, i1, i2, a.grad, c.grad)])
    _same_forward(outs[0][:4], outs[1][:4])
    _same_bits(outs[0][4], outs[1][4], "grad1")
    _same_bits(outs[0][5], outs[1][5], "grad2")


# ---- 3. layouts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 6])
@pytest.mark.parametrize("b,n,m", [(2, 300, T + 7), (1, 70, 33), (2, 1, 40)])
def test_layouts_agree_bit_for_bit(cuda, dim, b, n, m):
    x1, x2 = R.make_clouds(dim + n, b, n, m, dim)
    rng = np.random.default_rng(n)
    gd1 = torch.from_numpy(rng.standard_normal((b, n)).astype(np.float32)).to(cuda)
    gd2 = torch.from_numpy(rng.standard_normal((b, m)).astype(np.float32)).to(cuda)
    want = None
    for p1 in (False, True):
        for p2 in (False, True):
            a, c = _dev(x1, cuda, p1), _dev(x2, cuda, p2)
            if p1 and b > 1 and n > 1:
                assert not a.is_contiguous() and pcm_hip.cloud_layout_nd(a) == 1
            a.requires_grad_()
            c.requires_grad_()
            d1, d2, i1, i2 = ND.chamfer_NDDist()(a, c)
            ga, gc = torch.autograd.grad([d1, d2], [a, c], [gd1, gd2])
            # the gradients arrive in their input's layout
            assert pcm_hip.cloud_layout_nd(ga) == pcm_hip.cloud_layout_nd(a)
            assert pcm_hip.cloud_layout_nd(gc) == pcm_hip.cloud_layout_nd(c)
            got = [t.detach().cpu().numpy() for t in (d1, d2, i1, i2, ga, gc)]
            if want is None:
                want = got
                _same_forward(got[:4], R.forward_restated(x1, x2))
                r1, r2 = R.backward_restated(x1, x2, gd1.cpu().numpy(), gd2.cpu().numpy(), got[2], got[3])
                _same_bits(got[4], r1, "grad1, rows")
                _same_bits(got[5], r2, "grad2, rows")
            _same_forward(got[:4], want[:4], f"planes {p1} {p2}")
            _same_bits(got[4], want[4], f"grad1, planes {p1} {p2}")
            _same_bits(got[5], want[5], f"grad2, planes {p1} {p2}")


def test_raw_entries_in_planes(cuda):
    # the bindings themselves on channel planes, sentinels overwritten
    x1, x2 = R.make_clouds(77, 2, QB + 9, T + 5, 5)
    a, c = _dev(x1, cuda, True), _dev(x2, cuda, True)
    got = _forward(a, c, 1, 1)
    _same_forward(got, R.forward_restated(x1, x2))
    rng = np.random.default_rng(3)
    gd1, gd2 = rng.standard_normal(got[0].shape).astype(np.float32), rng.standard_normal(got[1].shape).astype(np.float32)
    g1, g2 = _backward(a, c, gd1, gd2, got[2], got[3], 1, 1)
    r1, r2 = R.backward_restated(x1, x2, gd1, gd2, got[2], got[3])
    _same_bits(g1, r1)
    _same_bits(g2, r2)


# ---- 4. ties ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 4, 8])
def test_ties_go_to_the_lowest_index(cuda, dim):
    rng = np.random.default_rng(dim)
    # a candidate cloud whose points are all equal
    x1 = R.make_cloud(rng, 1, QB + 3, dim)
    x2 = np.tile(R.make_cloud(rng, 1, 1, dim), (1, 2 * T + 3, 1))
    d1, d2, i1, i2 = _forward(_dev(x1, cuda), _dev(x2, cuda))
    assert np.all(i1 == 0)
    _same_forward((d1, d2, i1, i2), R.forward_restated(x1, x2))
    # copies of the true nearest point at k and k + T, and in each wave's share of one tile
    share = T // W
    for spots in ([5, 5 + T], [share - 1 + w * share for w in range(W)], [T + 3 + w * share for w in range(W)][::-1],
                  [T - 1, T, 2 * T + 2]):
        x2 = R.make_cloud(rng, 1, 2 * T + 3, dim, shift=2.0)  # far from the queries
        near = (x1[0, 7] + np.float32(0.015625)).astype(np.float32)
        x2[0, spots] = near
        got = _forward(_dev(x1, cuda), _dev(x2, cuda))
        assert got[2][0, 7] == min(spots)
        _same_forward(got, R.forward_restated(x1, x2), f"copies at {spots}")


# ---- 5. non-finite ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 8])
def test_non_finite_coordinates(cuda, dim):
    n, m = QB + 2, T + 5
    x1, x2 = R.make_clouds(dim, 2, n, m, dim)
    last = dim - 1
    x2[0, 0, 0] = NAN
    x2[0, T, last] = NAN
    x2[0, 3, 0] = INF
    x2[0, T + 1, last] = -INF
    x2[1, 0, last] = INF
    x2[1, T // W, 0] = NAN
    x1[0, 0, last] = NAN
    x1[0, 5, 0] = INF
    x1[0, QB, last] = -INF
    x1[1, 0, 0] = -INF
    x1[1, QB + 1, 0] = NAN
    want = R.forward_restated(x1, x2)
    assert np.isposinf(want[0][0, 0]) and want[2][0, 0] == 0  # a NaN query: (+inf, 0)
    _same_forward(_forward(_dev(x1, cuda), _dev(x2, cuda)), want)
    # an all-NaN candidate cloud
    allnan = np.full_like(x2, NAN)
    d1, d2, i1, i2 = _forward(_dev(x1, cuda), _dev(allnan, cuda))
    assert np.all(np.isposinf(d1)) and np.all(i1 == 0) and np.all(np.isposinf(d2)) and np.all(i2 == 0)
    # +-3e38: differences and squares that overflow
    y1, y2 = R.make_clouds(dim + 50, 2, n, m, dim)
    y1 = np.where(y1 >= 0.5, 3e38, -3e38).astype(np.float32)
    y2 = np.where(y2 >= 0.5, 3e38, -3e38).astype(np.float32)
    y2[1] = -np.abs(y2[1])
    y1[1] = np.abs(y1[1])  # element 1: every difference overflows
    want = R.forward_restated(y1, y2)
    assert np.all(np.isposinf(want[0][1])) and np.any(want[0][0] == 0)
    _same_forward(_forward(_dev(y1, cuda), _dev(y2, cuda)), want)


# ---- 6. backward -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 3, 6, 8])
def test_backward_collapsed_cloud(cuda, dim):
    # every one of 2 T + 3 sources lands on target 0; the ordered sum by a plain loop
    n, m = 2 * T + 3, QB + 1
    x1, x2 = R.make_clouds(dim + 9, 1, n, m, dim)
    rng = np.random.default_rng(dim)
    gd1, gd2 = rng.standard_normal((1, n)).astype(np.float32), rng.standard_normal((1, m)).astype(np.float32)
    i1 = np.zeros((1, n), np.int32)
    i2 = rng.integers(0, n, (1, m)).astype(np.int32)
    g1, g2 = _backward(_dev(x1, cuda), _dev(x2, cuda), gd1, gd2, i1, i2)
    f32 = np.float32
    acc = np.zeros(dim, f32)
    for j in range(n):
        acc = (acc + (-(f32(gd1[0, j] * f32(2.0)) * (x1[0, j] - x2[0, 0]).astype(f32)).astype(f32))).astype(f32)
    k = i2[0, 0]
    acc = (acc + (f32(gd2[0, 0] * f32(2.0)) * (x2[0, 0] - x1[0, k]).astype(f32)).astype(f32)).astype(f32)
    _same_bits(g2[0, 0], acc, "target 0 of the collapsed cloud")
    r1, r2 = R.backward_restated(x1, x2, gd1, gd2, i1, i2)
    _same_bits(g1, r1)
    _same_bits(g2, r2)


@pytest.mark.parametrize("dim", [2, 5, 8])
def test_backward_lattice_signed_zero_and_unused_output(cuda, dim):
    # lattice clouds; target t of cloud 1 is given 1 + t % 20 sources of cloud 2 until they run out, in shuffled
    # positions (the entry takes any indices inside the clouds)
    n, m = 2 * QB + 5, 3 * QB + 1
    rng = np.random.default_rng(dim)
    x1, x2 = R.make_clouds(dim + 60, 2, n, m, dim)
    a, c = _dev(x1, cuda), _dev(x2, cuda)
    owners = np.repeat(np.arange(n), 1 + np.arange(n) % 20)[:m].astype(np.int32)
    i2 = np.stack([rng.permutation(owners), rng.permutation(owners)])
    i1 = rng.integers(0, m, (2, n)).astype(np.int32)
    counts = np.bincount(i2[0], minlength=n)
    assert counts.max() == 20 and (counts == 1).any() and (counts == 0).any()
    gd1 = rng.standard_normal((2, n)).astype(np.float32)
    gd2 = rng.standard_normal((2, m)).astype(np.float32)
    gd1[:, ::5] = 0.0
    gd1[:, 1::5] = -0.0
    gd2[:, ::3] = -0.0
    gd2[:, 1::3] = -np.abs(gd2[:, 1::3])
    g1, g2 = _backward(a, c, gd1, gd2, i1, i2)
    r1, r2 = R.backward_restated(x1, x2, gd1, gd2, i1, i2)
    _same_bits(g1, r1)
    _same_bits(g2, r2)
    # one unused output: its graddist arrives as None and counts as zeros
    a.requires_grad_()
    c.requires_grad_()
    o1, _, j1, j2 = ND.chamfer_NDDist()(a, c)
    ga, gc = torch.autograd.grad([o1], [a, c], [torch.from_numpy(gd1).to(cuda)])
    r1, r2 = R.backward_restated(x1, x2, gd1, np.zeros_like(gd2), j1.cpu().numpy(), j2.cpu().numpy())
    _same_bits(ga.cpu().numpy(), r1)
    _same_bits(gc.cpu().numpy(), r2)


def test_backward_means_the_gradient(cuda):
    # float64 autograd of sum g1 d1 + sum g2 d2 through gathers with the kernel's own indices.  A component is a
    # sum of c terms; each term carries three float32 roundings (difference, g * 2 is exact, product; the
    # negation is exact) and the sum c more: |got - want| <= 2 (c + 3) 2^-24 sum |terms|, the 2 a margin
    dim, n, m = 6, QB + 40, 2 * QB + 3
    x1, x2 = R.make_clouds(4, 2, n, m, dim)
    d1, d2, i1, i2 = _forward(_dev(x1, cuda), _dev(x2, cuda))
    rng = np.random.default_rng(8)
    gd1, gd2 = rng.standard_normal((2, n)).astype(np.float32), rng.standard_normal((2, m)).astype(np.float32)
    g1, g2 = _backward(_dev(x1, cuda), _dev(x2, cuda), gd1, gd2, i1, i2)
    a = torch.from_numpy(x1).double().requires_grad_()
    c = torch.from_numpy(x2).double().requires_grad_()
    j1 = torch.from_numpy(i1).long()[..., None].expand(-1, -1, dim)
    j2 = torch.from_numpy(i2).long()[..., None].expand(-1, -1, dim)
    loss = (torch.from_numpy(gd1).double() * (a - c.gather(1, j1)).pow(2).sum(-1)).sum() \
        + (torch.from_numpy(gd2).double() * (c - a.gather(1, j2)).pow(2).sum(-1)).sum()
    loss.backward()
    # the terms' magnitudes and their number per component
    for got, want, self_, other, gs, go, i_s, i_o in ((g1, a.grad.numpy(), x1, x2, gd1, gd2, i1, i2),
                                                      (g2, c.grad.numpy(), x2, x1, gd2, gd1, i2, i1)):
        s64, o64 = self_.astype(np.float64), other.astype(np.float64)
        for bi in range(2):
            mag = np.abs(2.0 * gs[bi][:, None] * (s64[bi] - o64[bi][i_s[bi]]))
            cnt = np.ones(self_.shape[1])
            scat = np.abs(2.0 * go[bi][:, None] * (o64[bi] - s64[bi][i_o[bi]]))
            np.add.at(mag, i_o[bi], scat)
            np.add.at(cnt, i_o[bi], 1)
            bound = 2.0 * (cnt[:, None] + 3.0) * 2.0 ** -24 * mag
            assert np.all(np.abs(got[bi].astype(np.float64) - want[bi]) <= bound)


# ---- 7. sizes --------------------------------------------------------------------------------------------------

def test_empty_clouds_and_batches(cuda):
    dist = ND.chamfer_NDDist()
    for n, m in ((0, 5), (5, 0), (0, 0)):
        d1, d2, i1, i2 = dist(torch.rand(2, n, 4, device=cuda), torch.rand(2, m, 4, device=cuda))
        assert d1.shape == (2, n) and d2.shape == (2, m) and i1.dtype == torch.int32
        assert not d1.any() and not d2.any() and not i1.any() and not i2.any()
    d1, d2, i1, i2 = dist(torch.rand(0, 7, 4, device=cuda), torch.rand(0, 9, 4, device=cuda))
    assert d1.shape == (0, 7) and i2.shape == (0, 9)
    with pytest.raises(pcm_hip.PcmError):
        dist(torch.rand(1, pcm_hip.CHAMFER_ND_MAX_POINTS + 1, 2, device=cuda), torch.rand(1, 4, 2, device=cuda))


def test_largest_clouds_sampled(cuda):
    n, m, dim = pcm_hip.CHAMFER_ND_MAX_POINTS, pcm_hip.CHAMFER_ND_MAX_POINTS - 1, 8
    x1, x2 = R.make_clouds(12, 1, n, m, dim)
    d1, d2, i1, i2 = _forward(_dev(x1, cuda), _dev(x2, cuda))
    assert i1.min() >= 0 and i1.max() < m and i2.min() >= 0 and i2.max() < n
    rng = np.random.default_rng(2)
    for q, c, d, i in ((x1, x2, d1, i1), (x2, x1, d2, i2)):
        rows = np.sort(rng.choice(q.shape[1], 512, replace=False))
        rows[0], rows[-1] = 0, q.shape[1] - 1
        wd, wi = R.nn_restated(q, c, rows)
        np.testing.assert_array_equal(i[:, rows], wi)
        np.testing.assert_array_equal(R.bits(d[:, rows]), R.bits(wd))


# ---- 8. determinism and capture --------------------------------------------------------------------------------

def test_deterministic_and_capturable(cuda):
    dim, n, m = 5, QB + 30, T + 100
    x1, x2 = R.make_clouds(21, 2, n, m, dim)
    a, c = _dev(x1, cuda), _dev(x2, cuda, True)
    rng = np.random.default_rng(1)
    gd1 = torch.from_numpy(rng.standard_normal((2, n)).astype(np.float32)).to(cuda)
    gd2 = torch.from_numpy(rng.standard_normal((2, m)).astype(np.float32)).to(cuda)

    def buffers():
        return (torch.full((2, n), -1.0, device=cuda), torch.full((2, m), -1.0, device=cuda),
                torch.full((2, n), -7, dtype=torch.int32, device=cuda),
                torch.full((2, m), -7, dtype=torch.int32, device=cuda),
                torch.full((2, n, dim), NAN, device=cuda), _planes(torch.full((2, m, dim), NAN, device=cuda)))

    def step(o):
        pcm_hip.chamfer_nd_forward(a, 0, c, 1, o[0], o[1], o[2], o[3])
        pcm_hip.chamfer_nd_backward(a, 0, c, 1, gd1, gd2, o[2], o[3], o[4], o[5])

    runs = []
    for _ in range(2):
        o = buffers()
        step(o)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in o])
    o = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(o)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, fresh in zip(o, buffers()):
        t.copy_(fresh)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(o)
    graph.replay()
    torch.cuda.synchronize()
    runs.append([t.cpu().numpy() for t in o])
    for other in runs[1:]:
        _same_forward(other[:4], runs[0][:4])
        _same_bits(other[4], runs[0][4])
        _same_bits(other[5], runs[0][5])
    _same_forward(runs[0][:4], R.forward_restated(x1, x2))


# ---- 9. autograd -----------------------------------------------------------------------------------------------

def test_autograd_through_chamfer_6d_on_a_network_output(cuda):
    b, n, m = 2, 300, 257
    x1, x2 = R.make_clouds(33, b, n, m, 6)
    out = torch.from_numpy(np.ascontiguousarray(x1.transpose(0, 2, 1))).to(cuda).requires_grad_()  # [B, 6, N]
    gt = _dev(x2, cuda)
    d1, d2, i1, i2 = ND.chamfer_6DDist()(out.transpose(2, 1), gt)
    assert d1.dtype == torch.float32 and i1.dtype == torch.int32 and not i1.requires_grad
    (d1.mean() + d2.mean()).backward()
    assert out.grad.shape == (b, 6, n) and gt.grad is None
    w1, w2 = np.float32(1.0) / np.float32(b * n), np.float32(1.0) / np.float32(b * m)
    r1, _ = R.backward_restated(x1, x2, np.full((b, n), w1, np.float32), np.full((b, m), w2, np.float32),
                                i1.cpu().numpy(), i2.cpu().numpy())
    _same_forward([t.detach().cpu().numpy() for t in (d1, d2, i1, i2)], R.forward_restated(x1, x2))
    _same_bits(out.grad.cpu().numpy().transpose(0, 2, 1), r1)
    with pytest.raises(AssertionError, match="Wrong last dimension"):
        ND.chamfer_2DDist()(out.transpose(2, 1), gt)
