"""pcm_ball_query and pcm_uniform_loss on the GPU against the numpy restatement
of their contracts (tests/uniform_restated.py): index lists are EQUAL, the loss
is within one float32 rounding of the float64 restatement, the gradient within
the derived float32 bound, and both are bit-identical from run to run."""
import functools

import numpy as np
import pytest
import torch

import uniform_restated as U

pytestmark = pytest.mark.gpu

SMALL = [0.04, 0.08, 0.2]
DEFAULT = [0.004, 0.006, 0.008, 0.010, 0.012]
CASES = [(65, SMALL), (130, SMALL), (300, SMALL), (1024, DEFAULT)]
CASE_IDS = [f"n{n}" for n, _ in CASES]


def _planes(t):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(kind, n, b):
    """(xyz, params, restated dict, (grad, T, S)) of one input, computed once."""
    percentage = dict(CASES)[n]
    xyz = U.make_cloud(kind, 3, n, 100 + n)[:b]
    params = U.uniform_params(n, percentage)
    npoint, nsample, ball_radius, weight, L = params
    res = U.uniform_restated(xyz, npoint, nsample, ball_radius, weight, L)
    grad = U.uniform_gradient_f64(xyz, npoint, nsample, weight, L, res)
    return xyz, params, res, grad


def _run(dev_xyz, lay, params, want_grad=True, want_groups=True, workspace=None):
    import pcm_hip
    npoint, nsample, ball_radius, weight, L = params
    b = dev_xyz.shape[0]
    loss = torch.full((1,), -7.0, device=dev_xyz.device)
    grad = None
    if want_grad:
        grad = torch.full_like(dev_xyz, -7.0) if lay == 0 else \
            torch.full_like(dev_xyz.transpose(1, 2), -7.0).transpose(1, 2)
    groups = torch.full((b, npoint, sum(nsample)), -7, dtype=torch.int32, device=dev_xyz.device) if want_groups else None
    pcm_hip.uniform_loss(dev_xyz, lay, npoint, nsample, ball_radius, weight, L, loss, grad, groups,
                         workspace=workspace)
    return loss, grad, groups


# ---------------------------------------------------------------------------
# ball query
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_ball_query_equals_the_restatement(cuda, n):
    import pcm_hip
    rng = np.random.default_rng(7000 + n)
    b = 2
    xyz = rng.random((b, n, 3), dtype=np.float32)
    kinds = set()
    for s in (1, 3, 65):
        centres = (rng.random((b, s, 3), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)  # drawn on their own
        dx, dc = torch.from_numpy(xyz).to(cuda), torch.from_numpy(centres).to(cuda)
        for nsample in (1, 2, 12, 64):
            for radius in (0.05, 0.3, 0.8):
                want_i, want_c, hits = U.ball_query_restated(xyz, centres, radius, nsample)
                kinds |= {name for name, mask in (("empty", hits == 0), ("partly", (hits > 0) & (hits < nsample)),
                                                  ("over", hits > nsample)) if mask.any()}
                for lx in (0, 1):
                    for lc in (0, 1):
                        idx = torch.full((b, s, nsample), -7, dtype=torch.int32, device=cuda)
                        cnt = torch.full((b, s), -7, dtype=torch.int32, device=cuda)
                        vx, vc = _planes(dx) if lx else dx, _planes(dc) if lc else dc
                        # a cloud of one point is rows and planes at once: cloud_layout calls it rows
                        pcm_hip.ball_query(vx, pcm_hip.cloud_layout(vx), vc, pcm_hip.cloud_layout(vc), radius,
                                           nsample, idx, cnt)
                        np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
                        np.testing.assert_array_equal(cnt.cpu().numpy(), want_c)
    # empty, partly filled and over-full balls were all there (one point can only be alone or absent)
    assert kinds == ({"empty", "partly"} if n == 1 else {"empty", "partly", "over"})


def test_ball_query_is_strict_and_index_ordered(cuda):
    import pointnet2_utils as pn2
    inside = np.nextafter(np.float32(0.5), np.float32(0))
    cloud = np.array([[[0.5, 0, 0], [inside, 0, 0], [0, 0.5, 0], [0, 0, -0.5], [0, -inside, 0]]], np.float32)
    centre = np.zeros((1, 1, 3), np.float32)
    assert (np.float32(0.5) * np.float32(0.5)) == np.float32(0.25)  # d == r2 in float32: outside
    idx, cnt = pn2.ball_query_count(0.5, 4, torch.from_numpy(cloud).to(cuda), torch.from_numpy(centre).to(cuda))
    assert idx[0, 0].tolist() == [1, 4, 1, 1] and cnt[0, 0].item() == 2
    # a duplicated cloud: a point and its copy n apart, the list in index order and not by distance
    rng = np.random.default_rng(71)
    half = rng.random((2, 150, 3), dtype=np.float32)
    dup = np.concatenate([half, half], axis=1)
    centres = half[:, :9] + np.float32(0.01)
    want_i, want_c, hits = U.ball_query_restated(dup, centres, 0.25, 16)
    assert (hits % 2 == 0).all() and (hits > 16).any() and ((hits > 0) & (hits < 16)).any()
    idx, cnt = pn2.ball_query_count(0.25, 16, torch.from_numpy(dup).to(cuda), torch.from_numpy(centres).to(cuda))
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_c)
    real = np.arange(16)[None, None, :] < want_c[:, :, None]
    assert (np.diff(idx.cpu().numpy(), axis=2)[real[:, :, 1:]] > 0).all()
    assert torch.equal(pn2.ball_query(0.25, 16, torch.from_numpy(dup).to(cuda), torch.from_numpy(centres).to(cuda)),
                       idx)


def test_ball_query_non_finite_points_and_centres(cuda):
    import pointnet2_utils as pn2
    rng = np.random.default_rng(72)
    cloud = rng.random((2, 200, 3), dtype=np.float32)
    cloud[0, 0] = np.nan          # the first point: never the padding value by default
    cloud[0, 5, 1] = np.inf
    cloud[1, 70] = -np.inf
    cloud[1, 199, 2] = np.nan
    centres = rng.random((2, 6, 3), dtype=np.float32)
    centres[0, 2, 0] = np.nan     # a NaN centre: all zeros, count 0
    centres[1, 4] = np.inf
    want_i, want_c, _ = U.ball_query_restated(cloud, centres, 0.4, 32)
    idx, cnt = pn2.ball_query_count(0.4, 32, torch.from_numpy(cloud).to(cuda), torch.from_numpy(centres).to(cuda))
    got_i, got_c = idx.cpu().numpy(), cnt.cpu().numpy()
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_c, want_c)
    assert (got_i[0, 2] == 0).all() and got_c[0, 2] == 0 and (got_i[1, 4] == 0).all() and got_c[1, 4] == 0
    bad = {0: {0, 5}, 1: {70, 199}}
    for bi in range(2):
        for c in range(6):
            if got_c[bi, c]:
                assert not (set(got_i[bi, c].tolist()) & bad[bi])
    assert got_c.max() > 0 and ((got_i >= 0) & (got_i < 200)).all()


def test_grouping_follows_the_query(cuda):
    import pointnet2_utils as pn2
    rng = np.random.default_rng(73)
    cloud = torch.from_numpy(rng.random((2, 90, 3), dtype=np.float32)).to(cuda)
    seeds = pn2.furthest_point_sample(cloud, 7)
    assert seeds.dtype == torch.int32 and tuple(seeds.shape) == (2, 7)
    np.testing.assert_array_equal(seeds.cpu().numpy(), U.fps_restated(cloud.cpu().numpy(), 7))
    feats = cloud.transpose(1, 2).contiguous()
    new_xyz = pn2.gather_operation(feats, seeds).transpose(1, 2)  # a planes view, read in place
    idx = pn2.ball_query(0.3, 8, cloud, new_xyz)
    grouped = pn2.grouping_operation(feats, idx)
    assert tuple(grouped.shape) == (2, 3, 7, 8)
    want = U.gather_points(cloud.cpu().numpy(), idx.cpu().numpy())
    np.testing.assert_array_equal(grouped.permute(0, 2, 3, 1).cpu().numpy(), want)
    assert (idx[:, :, 0].long() <= seeds.long()).all()  # a seed is inside its own ball


# ---------------------------------------------------------------------------
# uniform loss
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["cube", "shell"])
@pytest.mark.parametrize("n,percentage", CASES, ids=CASE_IDS)
def test_uniform_loss_groups_loss_and_gradient(cuda, kind, n, percentage):
    # between the two clouds every size has padded, exactly full and truncated groups, and at the
    # default size the cube has groups that are one point repeated: conditions on the input
    kinds, single = set(), False
    for k2 in ("cube", "shell"):
        _, (npoint, nsample, _, _, _), res, _ = _case(k2, n, 3)
        for q, ns in enumerate(nsample):
            h = res["hits"][q]
            kinds |= {name for name, mask in (("padded", h < ns), ("full", h == ns), ("truncated", h > ns))
                      if mask.any()}
            single |= bool((h == 1).any())
    assert kinds == {"padded", "full", "truncated"} and (single or n != 1024)

    for b in (1, 3):
        xyz, params, res, (ref, count, mag) = _case(kind, n, b)
        npoint, nsample, ball_radius, weight, L = params
        dev = torch.from_numpy(xyz).to(cuda)
        loss, grad, groups = _run(dev, 0, params)
        want_groups = np.concatenate(res["groups"], axis=2)
        np.testing.assert_array_equal(groups.cpu().numpy(), want_groups)
        want = res["loss"]
        got = float(loss.item())
        print(f"{kind} n={n} b={b}: loss {got:.9g} restated {want:.9g} rel {abs(got - want) / abs(want):.3g}")
        # one float32 rounding, a factor two to spare; the double sums contribute about 1e-13
        assert abs(got - want) <= 2.0 ** -23 * abs(want)
        # the gradient over the kernel's own (= the restated) groups within the derived bound
        bound = U.gradient_bound(count, mag)
        gotg = grad.cpu().numpy().astype(np.float64)
        err = np.abs(gotg - ref)
        print(f"  gradient: largest error / bound {float((err / np.where(bound > 0, bound, 1.0)).max()):.3f}; "
              f"points with contributions {int((count > 0).sum())}, most per point {int(count.max())}")
        assert (err <= bound).all()
        assert (gotg[count == 0] == 0).all() and np.abs(ref).max() > 0
        # the loss alone, and without the lists: the same bits
        alone, none, _ = _run(dev, 0, params, want_grad=False, want_groups=False)
        assert none is None and torch.equal(_bits(alone), _bits(loss))
        # a planes view: the same lists and bits, the gradient written in planes
        loss_p, grad_p, groups_p = _run(_planes(dev), 1, params)
        assert grad_p.transpose(1, 2).is_contiguous()
        assert torch.equal(groups_p, groups) and torch.equal(_bits(loss_p), _bits(loss))
        assert torch.equal(_bits(grad_p), _bits(grad))


def test_the_most_scales_and_the_longest_groups(cuda):
    # eight scales, groups of 2 to 64 slots, 353 slots a seed: several passes of 64 slots, scales that
    # straddle them, the largest list storage a workgroup takes
    xyz = U.make_cloud("cube", 2, 600, 77)
    nsample = [2, 64, 33, 64, 64, 17, 64, 45]
    ball_radius = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.25]
    weight = [1.0, 0.5, 0.25, 2.0, 1.5, 0.125, 3.0, -0.75]
    params = (9, nsample, ball_radius, weight, 0.05)
    res = U.uniform_restated(xyz, *params)
    ref, count, mag = U.uniform_gradient_f64(xyz, 9, nsample, weight, 0.05, res)
    hits = np.stack(res["hits"], -1)
    assert (hits < nsample).any() and (hits > nsample).any()
    loss, grad, groups = _run(torch.from_numpy(xyz).to(cuda), 0, params)
    np.testing.assert_array_equal(groups.cpu().numpy(), np.concatenate(res["groups"], axis=2))
    # the scales' terms have both signs of weight: the bound is on their magnitudes
    size = sum(abs(w) * t.sum() for w, t in zip(weight, res["term"])) / (2 * 9)
    assert abs(loss.item() - res["loss"]) <= 2.0 ** -23 * size
    assert (np.abs(grad.cpu().numpy() - ref) <= U.gradient_bound(count, mag)).all() and np.abs(ref).max() > 0


def test_uniform_gradient_is_bit_identical_from_run_to_run(cuda):
    xyz, params, _, _ = _case("shell", 1024, 3)
    other, other_params, _, _ = _case("cube", 300, 3)
    dev, dev_other = torch.from_numpy(xyz).to(cuda), torch.from_numpy(other).to(cuda)
    loss, grad, groups = _run(dev, 0, params)
    loss2, grad2, groups2 = _run(dev, 0, params)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(grad), _bits(grad2))
    assert torch.equal(groups, groups2)
    # unrelated work on the stream, some of it through the same cached workspace
    _run(dev_other, 0, other_params)
    (torch.rand(512, 512, device=cuda) @ torch.rand(512, 512, device=cuda)).sum().item()
    loss3, grad3, _ = _run(dev, 0, params)
    assert torch.equal(_bits(loss), _bits(loss3)) and torch.equal(_bits(grad), _bits(grad3))


def test_zero_distance_slots_add_nothing(cuda):
    # eight points further apart than the largest ball, each sixteen times: every group is one point
    # repeated, every nearest other member a copy at distance zero -- the loss is that of m = 1e-8 and
    # no slot has a gradient (the reference's would be infinite)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    xyz = np.repeat(corners, 16, axis=0)[None].repeat(2, axis=0)
    xyz[1] = xyz[1, ::-1]
    params = U.uniform_params(128, SMALL)
    npoint, nsample, ball_radius, weight, L = params
    assert max(ball_radius) < 1
    res = U.uniform_restated(xyz, npoint, nsample, ball_radius, weight, L)
    ref, count, _ = U.uniform_gradient_f64(xyz, npoint, nsample, weight, L, res)
    assert all((e == 0).all() for e in res["e"]) and (ref == 0).all() and (count == 0).all()
    loss, grad, groups = _run(torch.from_numpy(xyz.copy()).to(cuda), 0, params)
    np.testing.assert_array_equal(groups.cpu().numpy(), np.concatenate(res["groups"], axis=2))
    assert abs(loss.item() - res["loss"]) <= 2.0 ** -23 * abs(res["loss"]) and res["loss"] > 0
    assert (grad == 0).all()


def test_non_finite_points_keep_every_index_in_range(cuda):
    # NaN and inf points are never hits but can be seeds (their running minimum never drops): such a seed's
    # groups are all zeros.  The call returns, the lists are the restatement's and in range, and the loss
    # follows IEEE from the contract (here a group of NaN points makes it non-finite); the gradient is
    # unspecified and only has to be written without a fault
    xyz = U.make_cloud("shell", 3, 130, 230).copy()
    xyz[0, 3] = np.nan
    xyz[1, 7, 0] = np.inf
    xyz[2, 0] = np.nan  # the first seed itself
    params = U.uniform_params(130, SMALL)
    with np.errstate(invalid="ignore", over="ignore"):
        res = U.uniform_restated(xyz, *params)
    loss, grad, groups = _run(torch.from_numpy(xyz).to(cuda), 0, params)
    got = groups.cpu().numpy()
    np.testing.assert_array_equal(got, np.concatenate(res["groups"], axis=2))
    assert ((got >= 0) & (got < 130)).all()
    assert (got[2, 0] == 0).all()
    want = res["loss"]
    assert not np.isfinite(want)
    assert (np.isnan(want) and np.isnan(loss.item())) or loss.item() == want
    # the finite clouds alone give a finite loss again through the same workspace
    clean = U.make_cloud("shell", 3, 130, 230)
    loss2, _, _ = _run(torch.from_numpy(clean).to(cuda), 0, params)
    assert abs(loss2.item() - _case("shell", 130, 3)[2]["loss"]) <= 2.0 ** -23 * loss2.item()


@pytest.mark.parametrize("kind", ["cube", "shell"])
def test_the_composed_path_gives_the_fused_loss(cuda, kind):
    import knn
    import pointnet2_utils as pn2
    n, b = 1024, 3
    xyz, params, res, _ = _case(kind, n, b)
    npoint, nsample, ball_radius, weight, L = params
    dev = torch.from_numpy(xyz).to(cuda)
    fused, _, _ = _run(dev, 0, params, want_grad=False, want_groups=False)
    feats = dev.transpose(1, 2).contiguous()
    seeds = pn2.furthest_point_sample(dev, npoint)
    new_xyz = pn2.gather_operation(feats, seeds).transpose(1, 2).contiguous()
    composed = 0.0
    for q, ns in enumerate(nsample):
        idx = pn2.ball_query(ball_radius[q], ns, dev, new_xyz)
        np.testing.assert_array_equal(idx.cpu().numpy(), res["groups"][q])
        grouped = pn2.grouping_operation(feats, idx).permute(0, 2, 3, 1).reshape(b * npoint, ns, 3).contiguous()
        d2, slots = knn.knn_points(grouped, grouped, 2)
        # the same neighbour slots and distance bits as the contract's restatement
        np.testing.assert_array_equal(slots[:, :, 1].cpu().numpy().reshape(b, npoint, ns), res["vstar"][q])
        e = d2[:, :, 1].cpu().numpy().reshape(b, npoint, ns)
        np.testing.assert_array_equal(e.view(np.int32), res["e"][q].view(np.int32))
        u, _ = U.u_values(e)  # finished on the host as the contract says
        m = u.astype(np.float64).sum(-1) / ns
        composed += weight[q] * ((m - L) ** 2 / (L + 1e-8)).sum() / (b * npoint)
    assert abs(fused.item() - composed) <= 2.0 ** -23 * abs(composed)


def test_loss_class_backpropagates(cuda):
    import loss as loss_mod
    import pcm_hip
    xyz, params, res, (ref, count, mag) = _case("shell", 1024, 3)
    dev = torch.from_numpy(xyz).to(cuda)
    want_loss, want_grad, _ = _run(dev, 0, params)
    rows = dev.clone().requires_grad_(True)
    value = loss_mod.Loss().get_uniform_loss(rows)
    assert value.dim() == 0 and value.requires_grad
    value.backward()
    assert torch.equal(_bits(value.detach().view(1)), _bits(want_loss)) and torch.equal(rows.grad, want_grad)
    assert (np.abs(rows.grad.cpu().numpy() - ref) <= U.gradient_bound(count, mag)).all()
    # a scaled upstream gradient, into the generator's [B, 3, N] layout without a copy
    gen_out = dev.transpose(1, 2).contiguous().requires_grad_(True)
    view = gen_out.transpose(2, 1)
    assert pcm_hip.cloud_layout(view) == 1
    (loss_mod.Loss().get_uniform_loss(view) * 3.0).backward()
    assert tuple(gen_out.grad.shape) == (3, 3, 1024) and gen_out.grad.is_contiguous()
    assert torch.equal(gen_out.grad.transpose(1, 2), 3.0 * want_grad)
    # no gradient wanted: none formed
    plain = loss_mod.Loss().get_uniform_loss(dev)
    assert not plain.requires_grad and torch.equal(_bits(plain.view(1)), _bits(want_loss))
    # other percentages and radius
    small = torch.from_numpy(_case("cube", 300, 3)[0]).to(cuda).requires_grad_(True)
    value = loss_mod.Loss().get_uniform_loss(small, percentage=SMALL, radius=1.0)
    assert abs(value.item() - _case("cube", 300, 3)[2]["loss"]) <= 2.0 ** -23 * value.item()
    # an empty batch: the mean over nothing (NaN, as torch.mean's) and an empty gradient
    empty = torch.empty(0, 1024, 3, device=cuda, requires_grad=True)
    value = loss_mod.Loss().get_uniform_loss(empty)
    assert torch.isnan(value).item()
    value.backward()
    assert tuple(empty.grad.shape) == (0, 1024, 3)


def test_python_errors_on_the_device(cuda):
    import loss as loss_mod
    import pcm_hip
    L = loss_mod.Loss()
    cloud = torch.rand(2, 100, 3, device=cuda)
    with pytest.raises(ValueError, match="0.004"):
        L.get_uniform_loss(cloud)  # nsample < 2
    with pytest.raises(ValueError, match="0.7"):
        L.get_uniform_loss(cloud, percentage=[0.04, 0.7])  # nsample > 64
    with pytest.raises(ValueError, match="0.05"):
        L.get_uniform_loss(torch.rand(2, 19, 3, device=cuda))  # N < 20: no seed
    with pytest.raises(RuntimeError):
        L.get_uniform_loss(cloud.cpu(), percentage=[0.04])
    with pytest.raises(TypeError):
        L.get_uniform_loss(cloud.double(), percentage=[0.04])
    # the library refuses what the Python layer lets through
    loss = torch.empty(1, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.uniform_loss(cloud, 0, 5, [4], [0.2], [1.0], 0.2, loss, workspace=torch.empty(8, dtype=torch.uint8,
                                                                                              device=cuda))
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.uniform_loss(cloud, 0, 5, [4], [-0.2], [1.0], 0.2, loss)


def test_uniform_graph_replay_equals_eager(cuda):
    import pcm_hip
    xyz, params, _, _ = _case("shell", 1024, 3)
    second = U.make_cloud("cube", 3, 1024, 9)
    npoint, nsample, ball_radius, weight, L = params
    eager = {}
    for name, c in (("first", xyz), ("second", second)):
        eager[name] = _run(torch.from_numpy(c).to(cuda), 0, params, want_groups=False)
    torch.cuda.synchronize()
    static = torch.from_numpy(xyz).to(cuda).clone()
    loss = torch.empty(1, device=cuda)
    grad = torch.empty_like(static)
    need = int(pcm_hip.load_library().pcm_uniform_workspace_bytes(3, 1024, npoint, len(nsample),
                                                                  pcm_hip._int_array(nsample)))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)

    def call():
        pcm_hip.uniform_loss(static, 0, npoint, nsample, ball_radius, weight, L, loss, grad, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one capture of loss plus gradient on a single stream
        call()
    for name, c in (("second", second), ("first", xyz)):
        static.copy_(torch.from_numpy(c).to(cuda))
        grad.fill_(-7)
        loss.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(loss), _bits(eager[name][0]))
        assert torch.equal(_bits(grad), _bits(eager[name][1]))
    # a workspace one byte short is refused
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.uniform_loss(static, 0, npoint, nsample, ball_radius, weight, L, loss, grad, workspace=ws[:-1])
