"""pcm_dcd_loss on the GPU against the numpy restatement of its contract
(tests/dcd_restated.py): count1_out / count2_out EQUAL to np.bincount of the
oracle's argmins, the loss, cd_p, cd_t and the graddists within the derived
float32 bounds, the gradients equal to the oracle's chamfer_backward fed the
call's own graddists; ties, non-finite input; bit-identity across runs,
layouts, batch positions and optional outputs; the autograd layer of
loss/dcd_loss.py and graph capture.

Largest error / bound observed on an MI355X over the 48 cases compared with
the restatement (the test prints the figures of every case): loss 0.20, cd
0.65, graddists 0.38 and 0.35; the gradients equal the oracle's bit for bit.
The comparison writes these ratios into the file PCM_DCD_RECORD names
(profiles/dcd/pytest_dcd_gpu.txt is such a record)."""
import os

import numpy as np
import pytest
import torch

import dcd_restated as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5  # tests/test_chamfer_gpu.py's tolerance of a gradient against the oracle's chamfer_backward
KEYS = ("loss", "cd", "g1", "g2", "c1", "c2", "gd1", "gd2")
_worst = {"loss": 0.0, "cd": 0.0, "graddist1": 0.0, "graddist2": 0.0, "gradient (absolute)": 0.0}


def _planes(t):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _like(t, lay):
    return torch.full_like(t, -7.0) if lay == 0 else torch.full_like(t.transpose(1, 2), -7.0).transpose(1, 2)


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.array(a)).to(cuda) for a in arrays]


def _run(x, y, alpha, lam=1.0, non_reg=False, cd=True, want1=True, want2=True, counts=True, gds=True, workspace=None):
    """dict(loss [B], cd, g1, g2, c1, c2, gd1, gd2) of one call (None where not
    asked for); each cloud in the layout it comes in; every output prefilled
    with a sentinel."""
    import pcm_hip
    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    l1, l2 = pcm_hip.cloud_layout(x), pcm_hip.cloud_layout(y)
    dev = x.device
    out = dict(loss=torch.full((b,), -7.0, device=dev), cd=torch.full((b, 2), -7.0, device=dev) if cd else None,
               g1=_like(x, l1) if want1 else None, g2=_like(y, l2) if want2 else None,
               c1=torch.full((b, n), -7, dtype=torch.int32, device=dev) if counts else None,
               c2=torch.full((b, m), -7, dtype=torch.int32, device=dev) if counts else None,
               gd1=torch.full((b, n), -7.0, device=dev) if gds else None,
               gd2=torch.full((b, m), -7.0, device=dev) if gds else None)
    pcm_hip.dcd_loss(x, l1, y, l2, float(alpha), float(lam), non_reg, out["loss"], out["cd"], out["g1"], out["g2"],
                     out["c1"], out["c2"], out["gd1"], out["gd2"], workspace=workspace)
    return out


def _same(a, b, names=KEYS):
    for k in names:
        if a[k] is not None and b[k] is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


def _compare(got, case, oracle, what):
    """One call's outputs against the restatement of its case."""
    x, y, d1, d2, i1, i2, alpha, res = case
    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    host = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.array_equal(host["c1"], res["c1"]), (what, "count1")
    assert np.array_equal(host["c2"], res["c2"]), (what, "count2")
    assert host["c1"].sum() == b * m and host["c2"].sum() == b * n
    bl, bc, b1, b2 = R.bounds(res, alpha, what[3], n, m)
    for name, key, want, bound in (("loss", "loss", res["loss"], bl), ("cd", "cd", res["cd"], bc),
                                   ("graddist1", "gd1", res["gd1"], b1), ("graddist2", "gd2", res["gd2"], b2)):
        err = np.abs(host[key].astype(np.float64) - want)
        ratio = float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)), initial=0.0))
        print(f"  {what} {name}: largest error {float(err.max()):.3g}, error / bound {ratio:.3g}")
        _worst[name] = max(_worst[name], ratio)
        assert (err <= bound).all(), (what, name, ratio)
    # the gradients: the oracle's deterministic backward on the call's own graddists
    r1, r2 = oracle.chamfer_backward(x, y, host["gd1"], host["gd2"], i1, i2)
    for name, value, want in (("gradxyz1", host["g1"], r1), ("gradxyz2", host["g2"], r2)):
        err = float(np.abs(value - want).max())
        print(f"  {what} {name}: largest error {err:.3g} (tolerance {TOL})")
        _worst["gradient (absolute)"] = max(_worst["gradient (absolute)"], err)
        np.testing.assert_allclose(value, want, rtol=0, atol=TOL)


@pytest.mark.parametrize("b,n,m,lam,non_reg", R.cases(),
                         ids=[f"b{b}-n{n}-m{m}-lambda{lam}-{'nonreg' if nr else 'reg'}" for b, n, m, lam, nr in R.cases()])
def test_counts_equal_and_values_within_bounds(cuda, oracle, b, n, m, lam, non_reg):
    case = R.restated(b, n, m, lam, non_reg)
    x, y, alpha, res = case[0], case[1], case[6], case[7]
    dx, dy = _dev(cuda, x, y)
    got = _run(dx, dy, alpha, lam, non_reg)
    _compare(got, case, oracle, (b, n, m, lam, non_reg))
    # the analytic gradient of the restatement: the float64 backward of the float64 graddists
    # (its graddists are within (a + 45) u of the call's, a < 100 here: 1e-4 of the largest component is ample)
    gx, gy = R.gradients(x, y, case[4], case[5], res["gd1"], res["gd2"])
    assert np.abs(got["g1"].cpu().numpy() - gx).max() <= TOL + 1e-4 * np.abs(gx).max()
    assert np.abs(got["g2"].cpu().numpy() - gy).max() <= TOL + 1e-4 * np.abs(gy).max()
    if n > 1 and m > 1:  # there is a loss and a gradient to miss
        assert np.abs(res["loss"]).min() > 1e-3 and np.abs(gx).max() * n > 1e-3


def test_record_largest_ratio():
    """After the comparison above (same process): the figures for profiles/dcd/."""
    print("largest error / bound:", _worst)
    if os.environ.get("PCM_DCD_RECORD") and max(_worst.values()) > 0:
        path = os.path.join(REPO, os.environ["PCM_DCD_RECORD"])
        with open(path, "w") as f:
            f.write("tests/test_dcd_gpu.py::test_counts_equal_and_values_within_bounds on "
                    f"{torch.cuda.get_device_name(0)}\nlargest error / bound over {len(R.cases())} cases "
                    "(counts equal in all):\n")
            for k, v in _worst.items():
                f.write(f"  {k}: {v:.4g}\n")


def test_ties_go_to_the_lower_index(cuda, oracle):
    """A target cloud whose second half repeats its first: every hit goes to
    the lower index and every duplicate's count is 0."""
    b, n, half = 2, 300, 77
    x, y = R.make_clouds(b, n, half, seed=5)
    y = np.ascontiguousarray(np.concatenate([y, y], axis=1))
    d1, d2, i1, i2 = oracle.chamfer_forward(x, y)
    assert i1.max() < half
    alpha = R.median_alpha(d1, d2)
    res = R.evaluate(d1, d2, i1, i2, alpha, 1.0, False)
    dx, dy = _dev(cuda, x, y)
    got = _run(dx, dy, alpha)
    c2 = got["c2"].cpu().numpy()
    assert not c2[:, half:].any() and c2[:, :half].sum() == b * n
    _compare(got, (x, y, d1, d2, i1, i2, alpha, res), oracle, (b, n, 2 * half, 1.0, False))
    # x duplicated as well: the duplicates of x are queries of their own, and targets never hit
    x2 = np.ascontiguousarray(np.concatenate([x, x], axis=1))
    d1, d2, i1, i2 = oracle.chamfer_forward(x2, y)
    res = R.evaluate(d1, d2, i1, i2, alpha, 0.5, True)
    got = _run(*_dev(cuda, x2, y), alpha, 0.5, True)
    assert not got["c1"].cpu().numpy()[:, n:].any() and not got["c2"].cpu().numpy()[:, half:].any()
    _compare(got, (x2, y, d1, d2, i1, i2, alpha, res), oracle, (b, 2 * n, 2 * half, 0.5, True))


def test_non_finite_input_stays_in_its_element(cuda, oracle):
    b, n, m = 3, 1000, 333
    x, y, d1, d2, i1, i2, alpha = R.forward(b, n, m)
    dx, dy = _dev(cuda, x, y)
    clean = _run(dx, dy, alpha)
    bad_x = x.copy()
    bad_x[1, 17, 0] = np.float32("nan")
    got = _run(_dev(cuda, bad_x)[0], dy, alpha)
    torch.cuda.synchronize()  # the call returned
    assert torch.isnan(got["loss"][1]).item()
    c1, c2 = got["c1"][1].cpu().numpy(), got["c2"][1].cpu().numpy()
    assert c1.min() >= 0 and c2.min() >= 0 and c1.sum() == m and c2.sum() == n  # every argmin stayed in range
    for i in (0, 2):
        for k in KEYS:
            assert torch.equal(_bits(got[k][i]), _bits(clean[k][i])), (k, i)
    # an infinite coordinate: that point is infinitely far from every target, so the query it decides (itself)
    # has e = 0: term 1 and graddist 0 exactly; everything else follows the restatement over the oracle's forward
    inf_x = x.copy()
    inf_x[1, 400, 2] = np.float32("inf")
    got = _run(_dev(cuda, inf_x)[0], dy, alpha, want1=False, want2=False)
    e1, e2, j1, j2 = oracle.chamfer_forward(inf_x, y)
    assert np.isinf(e1[1, 400]) and np.isfinite(np.delete(e1[1], 400)).all() and np.isfinite(e2).all()
    res = R.evaluate(e1, e2, j1, j2, alpha, 1.0, False)
    assert res["term1"][1, 400] == 1.0 and res["gd1"][1, 400] == 0.0
    assert np.array_equal(got["c1"].cpu().numpy(), res["c1"]) and np.array_equal(got["c2"].cpu().numpy(), res["c2"])
    assert got["gd1"][1, 400].item() == 0.0
    assert torch.isfinite(got["loss"]).all() and torch.isfinite(got["gd1"]).all() and torch.isfinite(got["gd2"]).all()
    assert torch.isinf(got["cd"][1]).all() and torch.isfinite(got["cd"][[0, 2]]).all()
    finite = dict(res, a1=res["a1"].copy())
    finite["a1"][1, 400] = 0.0  # its g is 0: the bound of that term is the final rounding alone
    bl, _, b1, b2 = R.bounds(finite, alpha, 1.0, n, m)
    assert (np.abs(got["loss"].cpu().numpy() - res["loss"]) <= bl).all()
    assert (np.abs(got["gd1"].cpu().numpy() - res["gd1"]) <= b1).all()
    assert (np.abs(got["gd2"].cpu().numpy() - res["gd2"]) <= b2).all()
    for i in (0, 2):
        for k in ("loss", "cd", "c1", "c2", "gd1", "gd2"):
            assert torch.equal(_bits(got[k][i]), _bits(clean[k][i])), (k, i)


def test_bit_identity(cuda):
    b, n, m = 3, 1000, 333
    x, y, _, _, _, _, alpha = R.forward(b, n, m)
    dx, dy = _dev(cuda, x, y)
    full = _run(dx, dy, alpha, 0.5, True)
    # unrelated work on the stream, some of it through the same cached workspace
    ox, oy = _dev(cuda, *R.make_clouds(1, 7, 5))
    _run(ox, oy, 3.0)
    (torch.rand(256, 256, device=cuda) @ torch.rand(256, 256, device=cuda)).sum().item()
    _same(full, _run(dx, dy, alpha, 0.5, True))
    # layouts
    for px in (False, True):
        for py in (False, True):
            got = _run(_planes(dx) if px else dx, _planes(dy) if py else dy, alpha, 0.5, True)
            assert got["g1"].transpose(1, 2).is_contiguous() if px else got["g1"].is_contiguous()
            assert got["g2"].transpose(1, 2).is_contiguous() if py else got["g2"].is_contiguous()
            _same(full, got)
    # every optional output NULL against present
    for kwargs in (dict(cd=False), dict(want1=False), dict(want2=False), dict(want1=False, want2=False),
                   dict(counts=False), dict(gds=False), dict(gds=False, want2=False),
                   dict(cd=False, want1=False, want2=False, counts=False, gds=False)):
        got = _run(dx, dy, alpha, 0.5, True, **kwargs)
        assert (got["g1"] is None) == (not kwargs.get("want1", True))
        _same(full, got)
    # element i alone equals element i of the batch
    for i in range(b):
        alone = _run(dx[i:i + 1].contiguous(), dy[i:i + 1].contiguous(), alpha, 0.5, True)
        for k in KEYS:
            assert torch.equal(_bits(alone[k][0]), _bits(full[k][i])), (k, i)


def test_every_output_is_overwritten(cuda):
    """Sentinels in every output, NaN bytes in the workspace: nothing of either survives."""
    import pcm_hip
    for b, n, m in ((2, 100, 33), (3, 7, 5), (2, 1025, 1023)):
        x, y, _, _, _, _, alpha = R.forward(b, n, m)
        dx, dy = _dev(cuda, x, y)
        want = _run(dx, dy, alpha)
        ws = torch.full((pcm_hip.dcd_workspace_bytes(b, n, m),), 255, dtype=torch.uint8, device=cuda)
        for px in (False, True):
            got = _run(_planes(dx) if px else dx, dy, alpha, workspace=ws)
            for k in KEYS:
                t = got[k]
                assert tuple(t.shape) == tuple(want[k].shape)
                assert not (t == -7).any().item(), k
                assert torch.isfinite(t).all().item() if t.is_floating_point() else (t >= 0).all().item(), k
            _same(want, got)


def test_autograd_layer(cuda):
    import dcd_loss
    import loss as loss_module
    import pcm_hip
    b, n, m = 3, 1000, 333
    x, y, d1, d2, i1, i2, alpha = R.forward(b, n, m)
    a = float(alpha)
    dx, dy = _dev(cuda, x, y)
    unit = _run(dx, dy, a, 0.5, True)
    # a non-uniform upstream weight per element: the unit gradients times the weights
    w = torch.tensor([0.5, -2.0, 3.0], device=cuda)
    px, py = dx.clone().requires_grad_(True), dy.clone().requires_grad_(True)
    value, cd = dcd_loss.dcd_lossFunction.apply(px, py, a, 0.5, True)
    assert tuple(value.shape) == (b,) and torch.equal(_bits(value.detach()), _bits(unit["loss"]))
    assert tuple(cd.shape) == (b, 2) and torch.equal(_bits(cd), _bits(unit["cd"])) and not cd.requires_grad
    (value * w).sum().backward()
    assert torch.equal(px.grad, w.view(b, 1, 1) * unit["g1"]) and torch.equal(py.grad, w.view(b, 1, 1) * unit["g2"])
    # calc_dcd: the published return, dist1 / idx1 belonging to gt's points
    px = dx.clone().requires_grad_(True)
    res = dcd_loss.calc_dcd(px, dy, alpha=a, n_lambda=0.5, return_raw=True, non_reg=True)
    assert len(res) == 7
    lossv, cd_p, cd_t, r_d1, r_d2, r_i1, r_i2 = res
    assert torch.equal(_bits(lossv.detach()), _bits(unit["loss"]))
    assert torch.equal(_bits(cd_p), _bits(unit["cd"][:, 0])) and torch.equal(_bits(cd_t), _bits(unit["cd"][:, 1]))
    assert not cd_p.requires_grad and not cd_t.requires_grad and lossv.requires_grad
    assert np.array_equal(r_d1.cpu().numpy(), d2) and np.array_equal(r_i1.cpu().numpy(), i2)  # gt's
    assert np.array_equal(r_d2.cpu().numpy(), d1) and np.array_equal(r_i2.cpu().numpy(), i1)
    assert len(dcd_loss.calc_dcd(dx, dy, alpha=a)) == 3
    # a cloud that does not require grad gets none, and none is formed for it
    lossv.sum().backward()
    assert dy.grad is None and torch.equal(px.grad, unit["g1"])
    value = dcd_loss.calc_dcd(dx, dy, alpha=a, n_lambda=0.5, non_reg=True)[0]
    assert not value.requires_grad and torch.equal(_bits(value), _bits(unit["loss"]))
    # the module and the training glue: the batch mean; the generator's [B, 3, N] output read in place
    mod = dcd_loss.DCDLoss(alpha=a, n_lambda=0.5, non_reg=True)(dx, dy)
    assert mod.dim() == 0 and torch.equal(mod, unit["loss"].mean())
    plain = _run(dx, dy, a)
    gen_out = dx.transpose(1, 2).contiguous().requires_grad_(True)
    view = gen_out.transpose(2, 1)
    assert pcm_hip.cloud_layout(view) == 1
    mean = loss_module.Loss().get_dcd_loss(view, dy, alpha=a)
    assert mean.dim() == 0 and torch.equal(mean.detach(), plain["loss"].mean())
    (mean * 6.0).backward()
    assert gen_out.grad.is_contiguous()
    assert torch.allclose(gen_out.grad.transpose(1, 2), plain["g1"] * (6.0 / b), rtol=1e-6, atol=0)
    # an empty batch
    empty = dcd_loss.calc_dcd(torch.empty(0, 8, 3, device=cuda), torch.empty(0, 9, 3, device=cuda))
    assert tuple(empty[0].shape) == (0,) and tuple(empty[1].shape) == (0,)


def test_python_errors_on_the_device(cuda):
    import pcm_hip
    x, y = torch.rand(2, 10, 3, device=cuda), torch.rand(2, 12, 3, device=cuda)
    loss = torch.empty(2, device=cuda)
    with pytest.raises(pcm_hip.PcmError):  # a workspace one byte short
        need = pcm_hip.dcd_workspace_bytes(2, 10, 12)
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, loss,
                         workspace=torch.empty(need, dtype=torch.uint8, device=cuda)[:-1])
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.dcd_loss(x, 0, y, 0, 0.0, 1.0, False, loss)
    with pytest.raises(pcm_hip.PcmError):  # more points than the library takes
        pcm_hip.dcd_loss(torch.rand(1, pcm_hip.DCD_MAX_POINTS + 1, 3, device=cuda), 0, y[:1], 0, 10.0, 1.0, False,
                         loss[:1])
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, torch.empty(1, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, loss, cd=torch.empty(2, 3, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, loss, gradxyz1=torch.empty(2, 12, 3, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, loss, count1=torch.empty(2, 10, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 0, y, 0, 10.0, 1.0, False, loss, graddist2=torch.empty(2, 10, device=cuda))
    with pytest.raises(ValueError):
        pcm_hip.dcd_loss(x, 1, y, 0, 10.0, 1.0, False, loss)


def test_graph_replay_equals_eager(cuda):
    import dcd_loss
    import pcm_hip
    b, n, m = 3, 1000, 333
    first, second = R.make_clouds(b, n, m, seed=3), R.make_clouds(b, n, m, seed=4)
    alpha = 40.0
    eager = [_run(*_dev(cuda, *c), alpha, 0.5) for c in (first, second)]
    torch.cuda.synchronize()
    sx, sy = _dev(cuda, *first)
    sx.requires_grad_(True)
    ws = torch.empty(pcm_hip.dcd_workspace_bytes(b, n, m), dtype=torch.uint8, device=cuda)
    out = {}

    def call():  # calc_dcd and its backward: forward, terms, Chamfer backward, two multiplies
        sx.grad = None
        res = dcd_loss.calc_dcd(sx, sy, alpha=alpha, n_lambda=0.5, workspace=ws)
        res[0].sum().backward()
        out["loss"], out["cd_p"], out["cd_t"], out["grad"] = res[0].detach(), res[1], res[2], sx.grad

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
        cx, cy = _dev(cuda, *clouds)
        with torch.no_grad():
            sx.copy_(cx)
            sy.copy_(cy)
            for t in out.values():
                t.fill_(-7)
        ws.fill_(255)  # the workspace needs no initialisation
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out["loss"]), _bits(want["loss"])), replay
        assert torch.equal(_bits(out["cd_p"]), _bits(want["cd"][:, 0]))
        assert torch.equal(_bits(out["cd_t"]), _bits(want["cd"][:, 1]))
        assert torch.equal(_bits(out["grad"]), _bits(want["g1"]))
