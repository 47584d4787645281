"""pcm_sinkhorn_loss on the GPU against the numpy float64 restatement of its
contract (tests/sinkhorn_restated.py): the loss, both gradients and the
potentials within TOL_LOSS / TOL_GRAD / TOL_POT for SHAPES x SETTINGS,
bit-identical across layouts, nullable gradients, runs and batch positions;
and the autograd layer of loss/sinkhorn_loss.py.

Largest error / tolerance observed on an MI355X over the 16 cases compared
with the restatement (the test prints the figures of every case): loss
1.6e-8 / 1e-6 = 0.016, normalised gradient 2.8e-6 / 1e-4 = 0.028, potentials
6.5e-7 / 1e-5 = 0.065 -- the hardware exp2 and log2 cost no more than numpy's
in the float32 restatement (1.4e-8, 2.2e-6, 1.0e-6 there)."""
import numpy as np
import pytest
import torch

import sinkhorn_restated as R

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"b{b}-n{n}-m{m}" for b, n, m in R.SHAPES]
BLUR, SCALING = R.SETTINGS[0]


def _planes(t):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _like(t, lay):
    return torch.full_like(t, -7.0) if lay == 0 else torch.full_like(t.transpose(1, 2), -7.0).transpose(1, 2)


def _run(x, y, blur=BLUR, scaling=SCALING, want1=True, want2=True, pots=False, workspace=None, diameter=R.DIAMETER):
    """(loss [B], grad_x or None, grad_y or None, potentials or None) of one
    pcm_sinkhorn_loss call; each cloud in the layout it comes in."""
    import pcm_hip
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    loss = torch.full((x.shape[0],), -7.0, device=x.device)
    g1 = _like(x, l1) if want1 else None
    g2 = _like(y, l2) if want2 else None
    p = torch.full((x.shape[0], x.shape[1] + y.shape[1], 2), -7.0, device=x.device) if pots else None
    pcm_hip.sinkhorn_loss(x, l1, y, l2, blur, scaling, diameter, loss, g1, g2, p, workspace=workspace)
    return loss, g1, g2, p


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.array(a)).to(cuda) for a in arrays]


def _check(got, want, tol, what, scale=1.0):
    err = scale * float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"  {what}: largest error {err:.3g}, tolerance {tol:.3g}, ratio {err / tol:.3f}")
    assert err <= tol, what


@pytest.mark.parametrize("blur,scaling", R.SETTINGS)
@pytest.mark.parametrize("b,n,m", R.SHAPES, ids=SHAPE_IDS)
def test_loss_gradients_and_potentials_within_tolerance(cuda, b, n, m, blur, scaling):
    x, y = R.make_clouds(b, n, m)
    want_l, want_gx, want_gy, want_p = R.restated(b, n, m, blur, scaling)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2, pots = _run(dx, dy, blur, scaling, pots=True)
    print(f"blur {blur} scaling {scaling} b{b} n{n} m{m}: loss {want_l[0]:.6g}")
    _check(loss.cpu().numpy(), want_l, R.TOL_LOSS, "loss")
    _check(g1.cpu().numpy(), want_gx, R.TOL_GRAD, "n grad x", scale=n)
    _check(g2.cpu().numpy(), want_gy, R.TOL_GRAD, "m grad y", scale=m)
    _check(pots.cpu().numpy(), want_p, R.TOL_POT, "potentials")
    # there is a loss and a gradient to miss
    assert want_l.min() > 1e4 * R.TOL_LOSS
    assert n * np.abs(want_gx).max() > 100 * R.TOL_GRAD and m * np.abs(want_gy).max() > 100 * R.TOL_GRAD


@pytest.mark.parametrize("b,n,m", [(2, 65, 63), (2, 300, 1025), (1, 1, 1)], ids=["small", "large", "one"])
def test_layouts_and_nullable_gradients_are_bit_identical(cuda, b, n, m):
    x, y = R.make_clouds(b, n, m)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2, pots = _run(dx, dy, pots=True)
    for px in (False, True):
        for py in (False, True):
            vx, vy = _planes(dx) if px else dx, _planes(dy) if py else dy
            for want1 in (True, False):
                for want2 in (True, False):
                    got_l, got1, got2, got_p = _run(vx, vy, want1=want1, want2=want2, pots=True)
                    assert torch.equal(_bits(got_l), _bits(loss)) and torch.equal(_bits(got_p), _bits(pots))
                    assert (got1 is None) == (not want1) and (got2 is None) == (not want2)
                    if want1:
                        # the gradient comes back in the cloud's layout (one point is rows and planes at once)
                        assert got1.transpose(1, 2).is_contiguous() if (px and n > 1) else got1.is_contiguous()
                        assert torch.equal(_bits(got1), _bits(g1))
                    if want2:
                        assert got2.transpose(1, 2).is_contiguous() if (py and m > 1) else got2.is_contiguous()
                        assert torch.equal(_bits(got2), _bits(g2))
    # potentials_out is optional too
    got_l, got1, got2, _ = _run(dx, dy, pots=False)
    assert torch.equal(_bits(got_l), _bits(loss)) and torch.equal(_bits(got1), _bits(g1))
    assert torch.equal(_bits(got2), _bits(g2))


def test_runs_and_batch_positions_are_bit_identical(cuda):
    x, y = R.make_clouds(3, 300, 1025, seed=3)
    dx, dy = _dev(cuda, x, y)
    loss, g1, g2, pots = _run(dx, dy, pots=True)
    # unrelated work on the stream, some of it through the same cached workspace
    other = _dev(cuda, *R.make_clouds(2, 65, 63))
    _run(other[0], other[1], 0.1, 0.7)
    (torch.rand(256, 256, device=cuda) @ torch.rand(256, 256, device=cuda)).sum().item()
    loss2, h1, h2, pots2 = _run(dx, dy, pots=True)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(g1), _bits(h1))
    assert torch.equal(_bits(g2), _bits(h2)) and torch.equal(_bits(pots), _bits(pots2))
    for i in range(3):  # element i alone equals element i of the batch
        li, a1, a2, pi = _run(dx[i:i + 1].contiguous(), dy[i:i + 1].contiguous(), pots=True)
        assert torch.equal(_bits(li), _bits(loss[i:i + 1])) and torch.equal(_bits(pi), _bits(pots[i:i + 1]))
        assert torch.equal(_bits(a1), _bits(g1[i:i + 1])) and torch.equal(_bits(a2), _bits(g2[i:i + 1]))


@pytest.mark.parametrize("blur,scaling", R.SETTINGS)
def test_roles_and_size_mismatch(cuda, blur, scaling):
    b, n, m = 2, 257, 255
    x, y = R.make_clouds(b, n, m)
    dx, dy = _dev(cuda, x, y)
    # x = y: the loss and every normalised gradient component within tolerance of 0
    loss, g1, g2, _ = _run(dx, dx.clone(), blur, scaling)
    assert loss.abs().max().item() <= R.TOL_LOSS
    assert n * g1.abs().max().item() <= R.TOL_GRAD and n * g2.abs().max().item() <= R.TOL_GRAD
    # the clouds' roles swapped: the same loss, the gradients and the potentials swapped bit for bit
    loss, g1, g2, pots = _run(dx, dy, blur, scaling, pots=True)
    loss_s, s1, s2, pots_s = _run(dy, dx, blur, scaling, pots=True)
    assert (loss - loss_s).abs().max().item() <= R.TOL_LOSS
    assert torch.equal(_bits(s1), _bits(g2)) and torch.equal(_bits(s2), _bits(g1))
    assert torch.equal(_bits(torch.cat([pots_s[:, m:], pots_s[:, :m]], 1)), _bits(pots))
    # n != m: y is x with every point twice -- the same measure
    twice = dx.repeat_interleave(2, dim=1)
    loss, g1, g2, _ = _run(dx, twice, blur, scaling)
    assert loss.abs().max().item() <= R.TOL_LOSS
    assert n * g1.abs().max().item() <= R.TOL_GRAD and 2 * n * g2.abs().max().item() <= R.TOL_GRAD


def test_a_nan_coordinate_stays_in_its_element(cuda):
    x, y = R.make_clouds(3, 65, 63)
    dx, dy = _dev(cuda, x, y)
    clean, c1, c2, _ = _run(dx, dy)
    for cloud, point in ((0, 64), (1, 0)):
        bad = [dx.clone(), dy.clone()]
        bad[cloud][1, point, 1] = float("nan")
        loss, g1, g2, _ = _run(bad[0], bad[1])
        torch.cuda.synchronize()  # the call returned
        assert torch.isnan(loss[1]).item()
        for i in (0, 2):
            assert torch.equal(_bits(loss[i:i + 1]), _bits(clean[i:i + 1]))
            assert torch.equal(_bits(g1[i]), _bits(c1[i])) and torch.equal(_bits(g2[i]), _bits(c2[i]))


def test_autograd_layer(cuda):
    import loss as loss_module
    import pcm_hip
    import sinkhorn_loss
    b, n, m = 3, 300, 1025
    x, y = R.make_clouds(b, n, m, seed=3)
    dx, dy = _dev(cuda, x, y)
    unit_l, unit1, unit2, _ = _run(dx, dy)
    L = sinkhorn_loss.SamplesLoss("sinkhorn", p=2, blur=BLUR, scaling=SCALING, diameter=R.DIAMETER)
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
    # diameter=None: the joint bounding box's larger extent, read back once
    auto = sinkhorn_loss.SamplesLoss("sinkhorn", blur=BLUR, scaling=SCALING)(dx, dy)
    box = float(np.float32(max(np.concatenate([x.reshape(-1, 3), y.reshape(-1, 3)]).max(0)
                               - np.concatenate([x.reshape(-1, 3), y.reshape(-1, 3)]).min(0))))
    assert sinkhorn_loss.joint_diameter(dx, dy) == box
    want = _run(dx, dy, diameter=box)[0]
    assert torch.equal(_bits(auto), _bits(want))
    # the generator's [B, 3, N] output as a transposed view: read in place, the gradient in planes
    gen_out = dx.transpose(1, 2).contiguous().requires_grad_(True)
    view = gen_out.transpose(2, 1)
    assert pcm_hip.cloud_layout(view) == 1
    mean = loss_module.Loss().get_sinkhorn_loss(view, dy, blur=BLUR, scaling=SCALING, diameter=R.DIAMETER)
    assert mean.dim() == 0 and torch.equal(mean.detach(), unit_l.mean())
    (mean * 6.0).backward()
    assert gen_out.grad.is_contiguous()
    assert torch.equal(gen_out.grad.transpose(1, 2), (torch.full((b,), 6.0, device=cuda) / b).view(b, 1, 1) * unit1)
    # the kernel norms delegate
    import kernel_loss
    assert torch.equal(sinkhorn_loss.SamplesLoss("energy")(dx, dy), kernel_loss.SamplesLoss("energy")(dx, dy))
    # an empty batch
    empty = L(torch.empty(0, 8, 3, device=cuda), torch.empty(0, 9, 3, device=cuda))
    assert tuple(empty.shape) == (0,)


def test_python_errors_on_the_device(cuda):
    import pcm_hip
    x, y = torch.rand(2, 10, 3, device=cuda), torch.rand(2, 12, 3, device=cuda)
    loss = torch.empty(2, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.sinkhorn_loss(x, 0, y, 0, -0.05, 0.5, 1.0, loss)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.sinkhorn_loss(x, 0, y, 0, 1e-3, 0.99, 1.0, loss)
    with pytest.raises(pcm_hip.PcmError):  # a workspace one byte short
        need = int(pcm_hip.load_library().pcm_sinkhorn_workspace_bytes(2, 10, 12))
        pcm_hip.sinkhorn_loss(x, 0, y, 0, 0.05, 0.5, 1.0, loss,
                              workspace=torch.empty(need, dtype=torch.uint8, device=cuda)[:-1])
    with pytest.raises(ValueError):
        pcm_hip.sinkhorn_loss(x, 0, y, 0, 0.05, 0.5, 1.0, torch.empty(1, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.sinkhorn_loss(x, 0, y, 0, 0.05, 0.5, 1.0, loss, gradxyz1=torch.empty(2, 12, 3, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.sinkhorn_loss(x, 0, y, 0, 0.05, 0.5, 1.0, loss, potentials=torch.empty(2, 22, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.sinkhorn_loss(x, 1, y, 0, 0.05, 0.5, 1.0, loss)


def test_graph_replay_equals_eager(cuda):
    import pcm_hip
    b, n, m = 3, 300, 1025
    first = R.make_clouds(b, n, m, seed=3)
    second = R.make_clouds(b, n, m, seed=4)
    eager = [_run(*_dev(cuda, *c)) for c in (first, second)]
    torch.cuda.synchronize()
    sx, sy = _dev(cuda, *first)
    loss = torch.empty(b, device=cuda)
    g1, g2 = torch.empty_like(sx), torch.empty_like(sy)
    ws = torch.empty(int(pcm_hip.load_library().pcm_sinkhorn_workspace_bytes(b, n, m)), dtype=torch.uint8,
                     device=cuda)

    def call():  # an explicit diameter: nothing is read back
        pcm_hip.sinkhorn_loss(sx, 0, sy, 0, BLUR, SCALING, R.DIAMETER, loss, g1, g2, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # T + 3 launches on a single stream
        call()
    for clouds, want in ((second, eager[1]), (first, eager[0])):
        cx, cy = _dev(cuda, *clouds)
        sx.copy_(cx)
        sy.copy_(cy)
        for t in (loss, g1, g2):
            t.fill_(-7)
        ws.fill_(255)  # the workspace needs no initialisation
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(loss), _bits(want[0]))
        assert torch.equal(_bits(g1), _bits(want[1])) and torch.equal(_bits(g2), _bits(want[2]))
