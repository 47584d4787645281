"""pcm_kernel_loss on the GPU against the numpy float64 restatement of its
contract (tests/kernel_loss_restated.py): the loss and both gradients within
the derived float32 bounds for the three kernels, bit-identical across layouts,
nullable gradients, runs and batch positions; and the autograd layer of
loss/kernel_loss.py.

Largest error / bound observed on an MI355X over the cases compared with the
restatement: loss 0.021, gradient 0.044 (the bounds add the worst case of every
rounding along a chain of up to 136 additions; DESIGN.md section 3.16 lists
them per kernel)."""
import numpy as np
import pytest
import torch

import kernel_loss_restated as R

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"b{b}-n{n}-m{m}" for b, n, m in R.SHAPES]


def _planes(t):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _like(t, lay):
    return torch.full_like(t, -7.0) if lay == 0 else torch.full_like(t.transpose(1, 2), -7.0).transpose(1, 2)


def _run(x, y, kernel, blur, want1=True, want2=True, workspace=None):
    """(loss [B], grad_x or None, grad_y or None) of one pcm_kernel_loss call;
    each cloud in the layout it comes in."""
    import pcm_hip
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((x.shape[0],), -7.0, device=x.device)
    g1 = _like(x, l1) if want1 else None
    g2 = _like(y, l2) if want2 else None
    pcm_hip.kernel_loss(x, l1, y, l2, kernel, blur, loss, g1, g2, workspace=workspace)
    return loss, g1, g2


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.array(a)).to(cuda) for a in arrays]


def _check(got, want, bound, what):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"  {what}: largest error {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3f}")
    assert err <= bound, what


@pytest.mark.parametrize("blur", R.BLURS)
@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
@pytest.mark.parametrize("b,n,m", R.SHAPES, ids=SHAPE_IDS)
def test_loss_and_gradients_within_the_bounds(cuda, b, n, m, kernel, blur):
    x, y = R.make_clouds(b, n, m)
    want_l, want_gx, want_gy = R.restated(b, n, m, kernel, blur)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2 = _run(dx, dy, kernel, blur)
    bx, by = R.grad_bound(kernel, n, m, blur)
    print(f"{R.KERNEL_NAMES[kernel]} blur {blur} b{b} n{n} m{m}: loss {want_l[0]:.6g}")
    _check(loss.cpu().numpy(), want_l, R.loss_bound(kernel, n, m, R.diameter(x, y)), "loss")
    _check(g1.cpu().numpy(), want_gx, bx, "grad x")
    _check(g2.cpu().numpy(), want_gy, by, "grad y")
    if n + m > 2:
        assert np.abs(want_gx).max() > 100 * bx and np.abs(want_gy).max() > 100 * by  # there is a gradient to miss


@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
@pytest.mark.parametrize("b,n,m", [(2, 65, 63), (2, 300, 1025), (1, 1, 1)], ids=["small", "large", "one"])
def test_layouts_and_nullable_gradients_are_bit_identical(cuda, b, n, m, kernel):
    x, y = R.make_clouds(b, n, m)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2 = _run(dx, dy, kernel, 0.2)
    for px in (False, True):
        for py in (False, True):
            vx, vy = _planes(dx) if px else dx, _planes(dy) if py else dy
            for want1 in (True, False):
                for want2 in (True, False):
                    got_l, got1, got2 = _run(vx, vy, kernel, 0.2, want1, want2)
                    assert torch.equal(_bits(got_l), _bits(loss))
                    assert (got1 is None) == (not want1) and (got2 is None) == (not want2)
                    if want1:
                        # the gradient comes back in the cloud's layout (one point is rows and planes at once)
                        assert got1.transpose(1, 2).is_contiguous() if (px and n > 1) else got1.is_contiguous()
                        assert torch.equal(_bits(got1), _bits(g1))
                    if want2:
                        assert got2.transpose(1, 2).is_contiguous() if (py and m > 1) else got2.is_contiguous()
                        assert torch.equal(_bits(got2), _bits(g2))


@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_runs_and_batch_positions_are_bit_identical(cuda, kernel):
    x, y = R.make_clouds(3, 300, 1025, seed=3)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2 = _run(dx, dy, kernel, 0.2)
    # unrelated work on the stream, some of it through the same cached workspace
    other = _dev(cuda, *R.make_clouds(2, 65, 63))
    _run(other[0], other[1], kernel, 1.0)
    (torch.rand(256, 256, device=cuda) @ torch.rand(256, 256, device=cuda)).sum().item()
    loss2, h1, h2 = _run(dx, dy, kernel, 0.2)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(g1), _bits(h1))
    assert torch.equal(_bits(g2), _bits(h2))
    for i in range(3):  # element i alone equals element i of the batch
        li, a1, a2 = _run(dx[i:i + 1].contiguous(), dy[i:i + 1].contiguous(), kernel, 0.2)
        assert torch.equal(_bits(li), _bits(loss[i:i + 1]))
        assert torch.equal(_bits(a1), _bits(g1[i:i + 1])) and torch.equal(_bits(a2), _bits(g2[i:i + 1]))


@pytest.mark.parametrize("blur", R.BLURS)
@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_roles_and_size_mismatch(cuda, kernel, blur):
    b, n, m = 2, 257, 255
    x, y = R.make_clouds(b, n, m)
    dx, dy = _dev(cuda, x, y)
    diam = R.diameter(x, y)
    # x = y: the loss and every gradient component within the bounds of 0
    loss, g1, g2 = _run(dx, dx.clone(), kernel, blur)
    bound = R.grad_bound(kernel, n, n, blur)[0]
    assert loss.abs().max().item() <= R.loss_bound(kernel, n, n, diam)
    assert g1.abs().max().item() <= bound and g2.abs().max().item() <= bound
    # the clouds' roles swapped: the same loss, the gradients swapped
    loss, g1, g2 = _run(dx, dy, kernel, blur)
    loss_s, s1, s2 = _run(dy, dx, kernel, blur)
    assert (loss - loss_s).abs().max().item() <= R.loss_bound(kernel, n, m, diam)
    assert torch.equal(_bits(s1), _bits(g2)) and torch.equal(_bits(s2), _bits(g1))
    # n != m: y is x with every point twice -- the same measure
    twice = dx.repeat_interleave(2, dim=1)
    loss, g1, g2 = _run(dx, twice, kernel, blur)
    assert loss.abs().max().item() <= R.loss_bound(kernel, n, 2 * n, diam)
    bx, by = R.grad_bound(kernel, n, 2 * n, blur)
    assert g1.abs().max().item() <= bx and g2.abs().max().item() <= by


@pytest.mark.parametrize("kernel", [R.LAPLACIAN, R.ENERGY], ids=R.KERNEL_NAMES.get)
def test_coincident_points_follow_the_subgradient_rule(cuda, kernel):
    rng = np.random.default_rng(21)
    base = rng.random((2, 40, 3), dtype=np.float32)
    x = np.concatenate([base, base[:, :25], base[:, 3:4].repeat(5, axis=1)], axis=1)  # 70 points, 30 repeats
    y = np.concatenate([rng.random((2, 50, 3), dtype=np.float32), base[:, 10:20]], axis=1)  # and 10 shared with x
    n, m = x.shape[1], y.shape[1]
    dx, dy = _dev(cuda, x, y)
    for blur in R.BLURS:
        loss, g1, g2 = _run(dx, dy, kernel, blur)
        assert torch.isfinite(loss).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all()
        res = [R.restated_one(x[i], y[i], kernel, blur) for i in range(2)]
        bx, by = R.grad_bound(kernel, n, m, blur)
        _check(loss.cpu().numpy(), np.array([r[0] for r in res]), R.loss_bound(kernel, n, m, R.diameter(x, y)), "loss")
        _check(g1.cpu().numpy(), np.stack([r[1] for r in res]), bx, "grad x")
        _check(g2.cpu().numpy(), np.stack([r[2] for r in res]), by, "grad y")
    # a cloud that is one point repeated, against itself: every pair coincides
    same = torch.from_numpy(base[:, :1].repeat(33, axis=1)).to(cuda)
    loss, g1, g2 = _run(same, same.clone(), kernel, 0.2)
    assert (loss == 0).all() and (g1 == 0).all() and (g2 == 0).all()


@pytest.mark.parametrize("kernel", R.KERNELS, ids=R.KERNEL_NAMES.get)
def test_a_nan_coordinate_stays_in_its_element(cuda, kernel):
    x, y = R.make_clouds(3, 65, 63)
    dx, dy = _dev(cuda, x, y)
    clean, c1, c2 = _run(dx, dy, kernel, 0.2)
    for cloud, point in ((0, 64), (1, 0)):
        bad = [dx.clone(), dy.clone()]
        bad[cloud][1, point, 1] = float("nan")
        loss, g1, g2 = _run(bad[0], bad[1], kernel, 0.2)
        torch.cuda.synchronize()  # the call returned
        assert torch.isnan(loss[1]).item()
        for i in (0, 2):
            assert torch.equal(_bits(loss[i:i + 1]), _bits(clean[i:i + 1]))
            assert torch.equal(_bits(g1[i]), _bits(c1[i])) and torch.equal(_bits(g2[i]), _bits(c2[i]))


def test_the_reference_blur_leaves_the_diagonal_and_no_gradient(cuda):
    g = torch.Generator().manual_seed(5)
    x, y = torch.rand(2, 64, 3, generator=g), torch.rand(2, 64, 3, generator=g)
    loss, g1, g2 = _run(x.to(cuda), y.to(cuda), R.GAUSSIAN, 5e-5)
    want = 0.5 * (1 / 64 + 1 / 64)
    assert (loss - want).abs().max().item() <= R.loss_bound(R.GAUSSIAN, 64, 64)
    assert (g1 == 0).all() and (g2 == 0).all()


def test_autograd_layer(cuda):
    import kernel_loss
    import pcm_hip
    b, n, m = 3, 300, 1025
    x, y = R.make_clouds(b, n, m, seed=3)
    dx, dy = _dev(cuda, x, y)
    for name, kernel in (("gaussian", R.GAUSSIAN), ("laplacian", R.LAPLACIAN), ("energy", R.ENERGY)):
        unit_l, unit1, unit2 = _run(dx, dy, kernel, 0.2)
        L = kernel_loss.SamplesLoss(name, blur=0.2)
        # a non-uniform upstream weight per element: the unit gradients times the weights
        w = torch.tensor([0.5, -2.0, 3.0], device=cuda)
        px, py = dx.clone().requires_grad_(True), dy.clone().requires_grad_(True)
        value = L(px, py)
        assert tuple(value.shape) == (b,) and torch.equal(_bits(value.detach()), _bits(unit_l))
        (value * w).sum().backward()
        assert torch.equal(px.grad, w.view(b, 1, 1) * unit1) and torch.equal(py.grad, w.view(b, 1, 1) * unit2)
        # a cloud that does not require grad gets none, and none is formed for it
        px = dx.clone().requires_grad_(True)
        value = L(px, dy)
        value.sum().backward()
        assert dy.grad is None and torch.equal(px.grad, unit1)
        value = L(dx, dy)
        assert not value.requires_grad and torch.equal(_bits(value), _bits(unit_l))
        # [N, 3] and [M, 3]: a scalar, the batched call's element
        p0, q0 = dx[1].clone().requires_grad_(True), dy[1].clone().requires_grad_(True)
        single = L(p0, q0)
        assert single.dim() == 0 and torch.equal(_bits(single.detach().view(1)), _bits(unit_l[1:2]))
        single.backward()
        assert torch.equal(p0.grad, unit1[1]) and torch.equal(q0.grad, unit2[1])
    # the generator's [B, 3, N] output as a transposed view: read in place, the gradient in planes
    unit_l, unit1, _ = _run(dx, dy, R.GAUSSIAN, 0.2)
    gen_out = dx.transpose(1, 2).contiguous().requires_grad_(True)
    view = gen_out.transpose(2, 1)
    assert pcm_hip.cloud_layout(view) == 1
    kernel_loss.SamplesLoss("gaussian", blur=0.2)(view, dy).sum().backward()
    assert gen_out.grad.is_contiguous() and torch.equal(gen_out.grad.transpose(1, 2), unit1)
    # batch_EMD_loss: the mean of the per-element values at the reference's blur
    per = kernel_loss.SamplesLoss("gaussian", p=2, blur=.00005)(dx, dy)
    mean = kernel_loss.batch_EMD_loss(dx, dy)
    assert mean.dim() == 0 and torch.equal(mean, per.mean())
    assert abs(mean.item() - 0.5 * (1 / n + 1 / m)) <= R.loss_bound(R.GAUSSIAN, n, m)
    # an empty batch
    empty = kernel_loss.SamplesLoss("energy")(torch.empty(0, 8, 3, device=cuda), torch.empty(0, 9, 3, device=cuda))
    assert tuple(empty.shape) == (0,)


def test_python_errors_on_the_device(cuda):
    import pcm_hip
    x, y = torch.rand(2, 10, 3, device=cuda), torch.rand(2, 12, 3, device=cuda)
    loss = torch.empty(2, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.kernel_loss(x, 0, y, 0, 0, -0.2, loss)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.kernel_loss(x, 0, y, 0, 3, 0.2, loss)
    with pytest.raises(pcm_hip.PcmError):  # a workspace one byte short
        need = int(pcm_hip.load_library().pcm_kernel_loss_workspace_bytes(2, 10, 12))
        pcm_hip.kernel_loss(x, 0, y, 0, 0, 0.2, loss, workspace=torch.empty(need, dtype=torch.uint8, device=cuda)[:-1])
    with pytest.raises(ValueError):
        pcm_hip.kernel_loss(x, 0, y, 0, 0, 0.2, torch.empty(1, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.kernel_loss(x, 0, y, 0, 0, 0.2, loss, gradxyz1=torch.empty(2, 12, 3, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.kernel_loss(x, 1, y, 0, 0, 0.2, loss)


def test_graph_replay_equals_eager(cuda):
    import pcm_hip
    b, n, m = 3, 300, 1025
    first = R.make_clouds(b, n, m, seed=3)
    second = R.make_clouds(b, n, m, seed=4)
    eager = [_run(*_dev(cuda, *c), R.GAUSSIAN, 0.2) for c in (first, second)]
    torch.cuda.synchronize()
    sx, sy = _dev(cuda, *first)
    loss = torch.empty(b, device=cuda)
    g1, g2 = torch.empty_like(sx), torch.empty_like(sy)
    ws = torch.empty(int(pcm_hip.load_library().pcm_kernel_loss_workspace_bytes(b, n, m)), dtype=torch.uint8,
                     device=cuda)

    def call():
        pcm_hip.kernel_loss(sx, 0, sy, 0, R.GAUSSIAN, 0.2, loss, g1, g2, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # loss plus both gradients on a single stream
        call()
    for clouds, want in ((second, eager[1]), (first, eager[0])):
        cx, cy = _dev(cuda, *clouds)
        sx.copy_(cx)
        sy.copy_(cy)
        for t in (loss, g1, g2):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(loss), _bits(want[0]))
        assert torch.equal(_bits(g1), _bits(want[1])) and torch.equal(_bits(g2), _bits(want[2]))
