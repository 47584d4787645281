"""Projection loss on the device: pcm_silhouette_forward / _backward and
pcm_proj_bce (csrc/silhouette.hip) and the Python layer above them
(utils/projection.py cont_proj, loss/proj_loss.py get_loss_proj).

Tolerances (none of them fitted to the code under test):
  forward   rtol 1e-4, atol 1e-30.  All terms are non-negative, so for any
            summation order the error is at most ((N - 1) 2^-24 + eps) value:
            6.1e-5 at N <= 1030, and eps <= 2e-5 covers two hardware
            exponentials of a scaled argument up to the underflow edge plus the
            product.  atol covers flushed denormal products, up to N 1.2e-38.
            (The reference's own float32 silhouette is within 3.5e-6 of
            float64, a sequential float32 sum within 7e-7.)
  backward  per point and coordinate |err| <= ((H W + 64) 2^-24 + 2e-5) A + 1e-30
            with A the same sum over the absolute values of its terms, in
            float64: the order-independent bound for H W mixed-sign terms.
  loss      (L + 8) 2^-24 mean|term| + 2.4e-7 with L = PCM_PROJ_BCE_CHAIN of
            include/pcm.h, the longest chain of additions (asserted <= 1024);
            grad_pred per element rtol 1e-6.
The float64 restatements start from the float32 co-ordinate map the contract
pins (gx = ((px + 1) H) / 2 in float32) and are float64 from there.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import silhouette_restated as R
from silhouette_restated import FWD_ATOL, FWD_RTOL, U, _bce_f64, _factors, _pinned, grad_f64, sil_f64

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "silhouette_golden.npz")
HEADER = os.path.join(REPO, "include", "pcm.h")

# the float64 references and the tolerance constants live in tests/silhouette_restated.py, shared with
# tests/test_silhouette_edges_cpu.py and tests/test_silhouette_edges_gpu.py


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(GOLDEN)
    cases = {}
    for i, name in enumerate(z["cases"]):
        cases[str(name)] = dict(xyz=z[f"{name}/xyz"], sil=z[f"{name}/sil"], grid=tuple(int(v) for v in z["grids"][i]),
                                sigma_sq=float(z["sigma_sq"][i]))
    return cases


@functools.lru_cache(maxsize=None)
def _case_f64(name):
    c = _fixture()[name]
    return sil_f64(c["xyz"], c["grid"][0], c["grid"][1], c["sigma_sq"])


@functools.lru_cache(maxsize=None)
def _case_grad(name):
    """(G float32 [B, H, W], float64 gradient, bound term A) of a fixture case, computed once."""
    c = _fixture()[name]
    b = c["xyz"].shape[0]
    G = torch.randn(b, c["grid"][0], c["grid"][1], generator=torch.Generator().manual_seed(17)).numpy()
    grad, A = grad_f64(c["xyz"], G, c["grid"][0], c["grid"][1], c["sigma_sq"])
    return G, grad, A


CASE_NAMES = ("finetune", "ragged", "one_point", "odd", "big_grid", "far")


# ---------------------------------------------------------------- direct calls


def _forward(x, grid_h, grid_w, sigma_sq, out=None):
    import pcm_hip
    if out is None:
        out = torch.empty(x.shape[0], grid_h, grid_w, device=x.device)
    pcm_hip.silhouette_forward(x, pcm_hip.cloud_layout(x), grid_h, grid_w, sigma_sq, out)
    return out


def _backward(x, G, grid_h, grid_w, sigma_sq, out=None):
    import pcm_hip
    lay = pcm_hip.cloud_layout(x)
    if out is None:
        b, n, _ = x.shape
        out = (torch.empty(b, 3, n, device=x.device).transpose(1, 2) if lay == 1
               else torch.empty(b, n, 3, device=x.device))
    pcm_hip.silhouette_backward(x, lay, grid_h, grid_w, sigma_sq, G, out)
    return out


def _planes(x):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rand_cloud(seed, b, n, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, n, 3, generator=g) * 2 - 1).to(dev)


# ---------------------------------------------------------------- forward


@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_matches_reference_and_float64(cuda, name):
    c = _fixture()[name]
    x = torch.from_numpy(c["xyz"]).to(cuda)
    got = _forward(x, c["grid"][0], c["grid"][1], c["sigma_sq"]).cpu().numpy().astype(np.float64)
    want = _case_f64(name)
    ref = c["sil"].astype(np.float64)
    print(f"{name}: max rel err vs float64 {np.max(np.abs(got - want) / np.maximum(want, 1e-300)):.3g}, "
          f"vs reference {np.max(np.abs(got - ref) / np.maximum(ref, 1e-300)):.3g}")
    np.testing.assert_allclose(got, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    np.testing.assert_allclose(got, ref, rtol=FWD_RTOL, atol=FWD_ATOL)


def test_cont_proj_matches_reference_through_the_python_layer(cuda):
    import projection
    c = _fixture()["ragged"]
    x = torch.from_numpy(c["xyz"]).to(cuda)
    out = projection.cont_proj(x, c["grid"][0], c["grid"][1], 'cpu', c["sigma_sq"])
    assert out.device == x.device and out.dtype == torch.float32 and tuple(out.shape) == c["sil"].shape
    assert _same_bits(out, _forward(x, c["grid"][0], c["grid"][1], c["sigma_sq"]))
    np.testing.assert_allclose(out.cpu().numpy(), c["sil"], rtol=FWD_RTOL, atol=FWD_ATOL)
    # default sigma_sq = 0.5, as the reference's signature
    assert _same_bits(projection.cont_proj(x, 8, 8, 'cuda'), _forward(x, 8, 8, 0.5))


@pytest.mark.parametrize("name", ["ragged", "finetune", "big_grid"])
def test_planes_give_the_same_bits_as_rows(cuda, name):
    import pcm_hip
    c = _fixture()[name]
    h, w = c["grid"]
    rows = torch.from_numpy(c["xyz"]).to(cuda)
    planes = _planes(rows)
    if rows.shape[1] > 1:
        assert pcm_hip.cloud_layout(rows) == 0 and pcm_hip.cloud_layout(planes) == 1
    assert _same_bits(_forward(rows, h, w, c["sigma_sq"]), _forward(planes, h, w, c["sigma_sq"]))
    G = torch.from_numpy(_case_grad(name)[0]).to(cuda)
    g_rows = _backward(rows, G, h, w, c["sigma_sq"])
    g_planes = _backward(planes, G, h, w, c["sigma_sq"])
    assert g_planes.stride() == planes.stride()
    assert _same_bits(g_rows, g_planes)


def test_forward_and_backward_are_deterministic_and_batch_independent(cuda):
    b, n, h, w, s2 = 33, 64, 8, 8, 0.5
    x = _rand_cloud(21, b, n, cuda)
    G = torch.randn(b, h, w, generator=torch.Generator().manual_seed(22)).to(cuda)
    s1, s2nd = _forward(x, h, w, s2), _forward(x, h, w, s2)
    g1, g2nd = _backward(x, G, h, w, s2), _backward(x, G, h, w, s2)
    assert _same_bits(s1, s2nd) and _same_bits(g1, g2nd)
    for i in (0, 7, 32):
        alone = _forward(x[i:i + 1].contiguous(), h, w, s2)
        assert _same_bits(alone[0], s1[i]), i
        g_alone = _backward(x[i:i + 1].contiguous(), G[i:i + 1].contiguous(), h, w, s2)
        assert _same_bits(g_alone[0], g1[i]), i
    # more than one chunk of points and more than one tile per cloud
    c = _fixture()["big_grid"]
    big = torch.from_numpy(c["xyz"]).to(cuda)
    stacked = torch.cat([_rand_cloud(23, 2, big.shape[1], cuda), big], 0)
    assert _same_bits(_forward(stacked, 128, 128, 2.0)[2], _forward(big, 128, 128, 2.0)[0])


@pytest.mark.parametrize("name", ["ragged", "odd", "big_grid"])
def test_outputs_are_fully_overwritten(cuda, name):
    c = _fixture()[name]
    h, w = c["grid"]
    x = torch.from_numpy(c["xyz"]).to(cuda)
    b, n, _ = x.shape
    sentinel = -12345.0
    out = torch.full((b, h, w), sentinel, device=cuda)
    _forward(x, h, w, c["sigma_sq"], out)
    assert not (out == sentinel).any() and _same_bits(out, _forward(x, h, w, c["sigma_sq"]))
    G = torch.from_numpy(_case_grad(name)[0]).to(cuda)
    for cloud in (x, _planes(x)):
        grad = torch.full_like(cloud, sentinel)  # keeps the cloud's layout
        assert grad.stride() == cloud.stride()
        _backward(cloud, G, h, w, c["sigma_sq"], grad)
        assert not (grad == sentinel).any()
        assert (_bits(grad[..., 2]) == 0).all()  # exactly +0


def test_non_finite_coordinates_follow_the_reference_sum(cuda):
    b, n, h, w, s2 = 3, 64, 8, 8, 0.5
    x = _rand_cloud(31, b, n, cuda)
    base = _forward(x, h, w, s2)
    # a NaN x poisons its own cloud only
    bad = x.clone()
    bad[1, 5, 0] = float("nan")
    out = _forward(bad, h, w, s2)
    assert torch.isnan(out[1]).all()
    assert _same_bits(out[0], base[0]) and _same_bits(out[2], base[2])
    # +inf y contributes 0: the cloud without that point
    inf = x.clone()
    inf[0, 7, 1] = float("inf")
    out = _forward(inf, h, w, s2)
    without = torch.cat([x[0:1, :7], x[0:1, 8:]], 1).contiguous()
    want = sil_f64(without.cpu().numpy(), h, w, s2)[0]
    assert torch.isfinite(out).all()
    np.testing.assert_allclose(out[0].cpu().numpy().astype(np.float64), want, rtol=FWD_RTOL, atol=FWD_ATOL)
    np.testing.assert_allclose(out[0].cpu().numpy(), _forward(without, h, w, s2)[0].cpu().numpy(),
                               rtol=2 * FWD_RTOL, atol=FWD_ATOL)
    assert _same_bits(out[1:], base[1:])
    ninf = x.clone()
    ninf[2, 0, 0] = float("-inf")
    assert torch.isfinite(_forward(ninf, h, w, s2)).all()
    # z is never read
    zz = x.clone()
    zz[:, ::3, 2] = float("nan")
    zz[0, 1, 2] = float("inf")
    assert _same_bits(_forward(zz, h, w, s2), base)
    assert _same_bits(_forward(_planes(zz), h, w, s2), base)


# ---------------------------------------------------------------- backward


@pytest.mark.parametrize("name", ["ragged", "odd", "finetune", "big_grid"])
def test_backward_matches_float64_autograd(cuda, name):
    c = _fixture()[name]
    h, w = c["grid"]
    G, want, A = _case_grad(name)
    x = torch.from_numpy(c["xyz"]).to(cuda)
    got = _backward(x, torch.from_numpy(G).to(cuda), h, w, c["sigma_sq"]).cpu().numpy().astype(np.float64)
    bound = ((h * w + 64) * U + 2e-5) * A + 1e-30
    err = np.abs(got[..., :2] - want[..., :2])
    print(f"{name}: max err / bound {np.max(err / bound):.3g}; max err / A {np.max(err / np.maximum(A, 1e-300)):.3g}")
    assert (err <= bound).all()
    assert (got[..., 2] == 0).all()


# ---------------------------------------------------------------- pcm_proj_bce


def _bce_chain():
    src = open(HEADER).read()
    return int(re.search(r"#define\s+PCM_PROJ_BCE_CHAIN\s+(\d+)", src).group(1))


@pytest.mark.parametrize("w", [1.0, 0.5])
@pytest.mark.parametrize("count", R.BCE_COUNTS + R.BCE_NEW_COUNTS)
def test_proj_bce_loss_and_gradient(cuda, count, w):
    # the new counts: the two sides of the single-workgroup switch (2048 / 2049), the last count whose
    # partials fit one trip of the finalise kernel's strided loop (524288 = 256 workgroups), the first that
    # takes a second (524289), 257 full workgroups, and 2^20, the largest count PCM_PROJ_BCE_CHAIN covers.
    # gt = rand are probabilities; gt = rand * 3 are silhouette targets, above 1 where points overlap.
    import pcm_hip
    L = _bce_chain()
    assert L <= 1024 and count <= 2 ** 20
    for gt_scale in R.BCE_GT_SCALES:
        pred, gt = R.bce_inputs(count, gt_scale)
        term, grad = _bce_f64(pred.numpy(), gt.numpy(), w)
        want = term.sum() / float(np.float32(count))
        tol = (L + 8) * U * np.mean(np.abs(term)) + 2.4e-7
        p, t = pred.to(cuda), gt.to(cuda)
        loss = torch.full((1,), float("nan"), device=cuda)
        gp = torch.full((count,), float("nan"), device=cuda)
        pcm_hip.proj_bce(p, t, w, loss, gp)
        got = float(loss.item())
        print(f"count {count} w {w} gt x{gt_scale:g}: loss {got!r} want {want!r} |err| {abs(got - want):.3g} "
              f"tol {tol:.3g} err/tol {abs(got - want) / tol:.3g}; "
              f"grad max rel err {np.max(np.abs(gp.cpu().numpy() - grad) / np.abs(grad)):.3g}")
        R.note("bce", count, gt_scale, abs(got - want) / tol)
        assert abs(got - want) <= tol
        np.testing.assert_allclose(gp.cpu().numpy().astype(np.float64), grad, rtol=1e-6, atol=0)
        # grad_pred = NULL is accepted and leaves the loss bit for bit the same; so does a second run
        loss2 = torch.full((1,), float("nan"), device=cuda)
        pcm_hip.proj_bce(p, t, w, loss2, None)
        assert _same_bits(loss, loss2)
        gp2 = torch.empty_like(gp)
        pcm_hip.proj_bce(p, t, w, loss2, gp2)
        assert _same_bits(loss, loss2) and _same_bits(gp, gp2)
        if count > 2048:  # more than one workgroup: the partials go through the workspace, whatever it held
            need = pcm_hip.load_library().pcm_proj_bce_workspace_bytes(count)
            assert need >= 4 * ((count + 2047) // 2048)
            junk = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)  # NaN bit patterns
            for _ in range(2):
                loss3 = torch.full((1,), float("nan"), device=cuda)
                pcm_hip.proj_bce(p, t, w, loss3, None, workspace=junk)
                assert _same_bits(loss, loss3)


@pytest.mark.parametrize("w", [1.0, 0.5])
def test_proj_bce_edge_values_per_element(cuda, w):
    """R.bce_edge_vector, one element a call (count = 1: the loss is the element's term, the gradient its
    derivative), so that a log(1e-8) term cannot hide its neighbours in a sum."""
    import pcm_hip
    L = _bce_chain()
    preds, gts = R.bce_edge_vector()
    assert preds.size == 28
    term, _ = _bce_f64(preds, gts, w)
    assert np.isfinite(term).all()
    worst = 0.0
    for k in range(preds.size):
        want, grad = _bce_f64(preds[k:k + 1], gts[k:k + 1], w)
        tol = (L + 8) * U * abs(want[0]) + 2.4e-7
        loss = torch.full((1,), float("nan"), device=cuda)
        gp = torch.full((1,), float("nan"), device=cuda)
        p, t = torch.from_numpy(preds[k:k + 1]).to(cuda), torch.from_numpy(gts[k:k + 1]).to(cuda)
        pcm_hip.proj_bce(p, t, w, loss, gp)
        got, got_g = float(loss.item()), float(gp.item())
        worst = max(worst, abs(got - want[0]) / tol)
        assert abs(got - want[0]) <= tol, (preds[k], gts[k], got, want[0])
        assert abs(got_g - grad[0]) <= 1e-6 * abs(grad[0]), (preds[k], gts[k], got_g, grad[0])
    print(f"edge vector w {w}: worst |err| / tol {worst:.3g}")
    # the whole vector in one call: the same terms through the workgroup's sum
    want = term.sum() / float(np.float32(preds.size))
    loss = torch.full((1,), float("nan"), device=cuda)
    pcm_hip.proj_bce(torch.from_numpy(preds).to(cuda), torch.from_numpy(gts).to(cuda), w, loss, None)
    assert abs(float(loss.item()) - want) <= (L + 8) * U * np.mean(np.abs(term)) + 2.4e-7


# ---------------------------------------------------------------- autograd


def _by_hand(pred_cloud, gt_cloud, h, w, s2, weight=1.0):
    """The three entries chained by hand: (loss, gradient for pred_cloud)."""
    import pcm_hip
    S = _forward(pred_cloud, h, w, s2)
    T = _forward(gt_cloud, h, w, s2)
    loss = torch.empty((), device=S.device)
    gS = torch.empty_like(S)
    pcm_hip.proj_bce(S, T, weight, loss, gS)
    return loss, _backward(pred_cloud, gS, h, w, s2)


def test_cont_proj_autograd_equals_direct_calls(cuda):
    import projection
    c = _fixture()["ragged"]
    h, w = c["grid"]
    G = torch.from_numpy(_case_grad("ragged")[0]).to(cuda)
    for make in (lambda t: t, _planes):
        x = make(torch.from_numpy(c["xyz"]).to(cuda)).detach().requires_grad_()
        S = projection.cont_proj(x, h, w, 'cuda', c["sigma_sq"])
        S.backward(G)
        assert _same_bits(S, _forward(x.detach(), h, w, c["sigma_sq"]))
        assert _same_bits(x.grad, _backward(x.detach(), G, h, w, c["sigma_sq"]))
    # through perspective_transform's view of planes, as utils/utils.py:228-232 chains them
    cam = torch.from_numpy(c["xyz"]).to(cuda)
    cam[:, :, 2] += 2.5
    persp = projection.perspective_transform(cam, 'cuda', cam.shape[0])
    import pcm_hip
    assert pcm_hip.cloud_layout(persp) == 1
    scaled = (persp / 64.0).detach()  # a view of planes stays one under elementwise ops
    assert pcm_hip.cloud_layout(scaled) == 1
    assert _same_bits(projection.cont_proj(scaled, h, w, 'cuda', 2.0), _forward(scaled.contiguous(), h, w, 2.0))


def test_projection_loss_autograd_equals_the_three_entries_by_hand(cuda):
    import proj_loss
    import projection
    b, n, h, w, s2 = 2, 200, 16, 24, 2.0
    pred_cloud = _rand_cloud(51, b, n, cuda).requires_grad_()
    gt_cloud = _rand_cloud(52, b, n, cuda)
    loss, fwd, bwd = proj_loss.get_loss_proj(projection.cont_proj(pred_cloud, h, w, 'cuda', s2),
                                             projection.cont_proj(gt_cloud, h, w, 'cuda', s2).detach(), 'cuda',
                                             'bce_prob')
    assert fwd is None and bwd is None and loss.dim() == 0
    loss.backward()
    want_loss, want_grad = _by_hand(pred_cloud.detach(), gt_cloud, h, w, s2)
    assert _same_bits(loss, want_loss)
    assert _same_bits(pred_cloud.grad, want_grad)


@pytest.mark.parametrize("seed", [65, 126])
def test_composed_path_matches_float64_autograd(cuda, seed):
    import proj_loss
    import projection
    b, n, h, w, s2 = 2, 48, 8, 8, 0.5
    g = torch.Generator().manual_seed(seed)
    pred_cpu = torch.rand(b, n, 3, generator=g) * 2 - 1
    gt_cpu = torch.rand(b, n, 3, generator=g) * 2 - 1
    # float64: silhouettes from the pinned co-ordinates, the loss, autograd to the co-ordinates
    gx, gy = _pinned(pred_cpu.numpy(), h, w)
    tx, ty = torch.from_numpy(gx).requires_grad_(), torch.from_numpy(gy).requires_grad_()
    cells_h, cells_w = torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64)
    ex = torch.exp(-(tx[..., None] - cells_h) ** 2 / (2.0 * s2))
    ey = torch.exp(-(ty[..., None] - cells_w) ** 2 / (2.0 * s2))
    S = torch.einsum("bnh,bnw->bhw", ex, ey)
    T = torch.from_numpy(sil_f64(gt_cpu.numpy(), h, w, s2))
    mu = float((S.detach() - 1).abs().min())
    p_max = float(S.detach().max())
    print(f"seed {seed}: margin {mu:.4g}, largest predicted cell {p_max:.4g}")
    assert mu >= 0.05
    S.retain_grad()
    loss64 = (-T * torch.log(S + 1e-8) - (1 - T) * torch.log(torch.abs(1 - S - 1e-8))).mean()
    loss64.backward()
    want = np.stack([tx.grad.numpy() * (h / 2.0), ty.grad.numpy() * (w / 2.0)], -1)
    dx, nex = _factors(gx, h, s2)
    dy, ney = _factors(gy, w, s2)
    aG = S.grad.abs().numpy()
    A = np.stack([np.einsum("bnh,bnw,bhw->bn", np.abs(dx / s2) * nex, ney, aG) * (h / 2.0),
                  np.einsum("bnh,bnw,bhw->bn", nex, np.abs(dy / s2) * ney, aG) * (w / 2.0)], -1)
    # the device
    pred_cloud = pred_cpu.to(cuda).requires_grad_()
    loss = proj_loss.get_loss_proj(projection.cont_proj(pred_cloud, h, w, 'cuda', s2),
                                   projection.cont_proj(gt_cpu.to(cuda), h, w, 'cuda', s2).detach(), 'cuda',
                                   'bce_prob')[0]
    loss.backward()
    got = pred_cloud.grad.cpu().numpy().astype(np.float64)
    tol = (1e-4 * p_max / mu + 3e-4) * A
    err = np.abs(got[..., :2] - want)
    print(f"seed {seed}: loss {float(loss.detach()):.9g} float64 {float(loss64.detach()):.9g}; "
          f"max err / tol {np.max(err / tol):.3g}")
    assert (err <= tol).all()
    assert (got[..., 2] == 0).all()
    # the loss itself: a 1e-4 relative error of a silhouette cell moves log|1 - S| by at most
    # 1e-4 p_max / mu and log(S), like the gt cell's own weight, by 1e-4; then the sum's bound
    T_np, S_np = T.numpy(), S.detach().numpy()
    term = np.abs(T_np * np.log(S_np + 1e-8)) + np.abs((1 - T_np) * np.log(np.abs(1 - S_np - 1e-8)))
    loss_tol = (1e-4 * (p_max / mu) * np.mean(np.abs(1 - T_np) + np.abs(T_np)) + 2e-4 * np.mean(term)
                + (_bce_chain() + 8) * U * np.mean(term) + 2.4e-7)
    assert abs(float(loss.detach()) - float(loss64.detach())) <= loss_tol


def test_graph_replay_equals_eager(cuda):
    import proj_loss
    import projection
    b, n, h, w, s2 = 4, 300, 16, 24, 2.0
    first, second = _rand_cloud(61, b, n, cuda), _rand_cloud(62, b, n, cuda)
    gt_cloud = _rand_cloud(63, b, n, cuda)
    static = first.clone().requires_grad_()

    def step():
        static.grad = None
        S = projection.cont_proj(static, h, w, 'cuda', s2)
        T = projection.cont_proj(gt_cloud, h, w, 'cuda', s2).detach()
        loss = proj_loss.get_loss_proj(S, T, 'cuda', 'bce_prob')[0]
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    static.grad = None
    with torch.cuda.graph(graph):
        captured_loss = step()
    for cloud in (first, second):
        with torch.no_grad():
            static.copy_(cloud)
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_grad = _by_hand(cloud, gt_cloud, h, w, s2)
        assert _same_bits(captured_loss, want_loss)
        assert _same_bits(static.grad, want_grad)


# ---------------------------------------------------------------- full shape


def test_full_finetune_shape_spot_checked_against_float64(cuda):
    b, n, h, w, s2 = 32, 1024, 64, 64, 2.0
    x = _rand_cloud(71, b, n, cuda)
    out = _forward(x, h, w, s2)
    assert tuple(out.shape) == (b, h, w) and torch.isfinite(out).all()
    gx, gy = _pinned(x.cpu().numpy(), h, w)
    cells = torch.randint(0, h * w, (b, 4), generator=torch.Generator().manual_seed(72)).numpy()
    host = out.cpu().numpy().astype(np.float64)
    for i in range(b):
        for cell in cells[i]:
            ch, cw = int(cell) // w, int(cell) % w
            want = np.sum(np.exp(-(gx[i] - ch) ** 2 / (2 * s2)) * np.exp(-(gy[i] - cw) ** 2 / (2 * s2)))
            assert abs(host[i, ch, cw] - want) <= FWD_RTOL * want + FWD_ATOL, (i, ch, cw)
    # the backward's launch geometry at the same shape: finite, z exactly 0, planes as rows
    G = torch.randn(b, h, w, generator=torch.Generator().manual_seed(73)).to(cuda)
    grad = _backward(x, G, h, w, s2)
    assert torch.isfinite(grad).all() and (_bits(grad[..., 2]) == 0).all()
    assert _same_bits(grad, _backward(_planes(x), G, h, w, s2))
