"""pcm_knn and pcm_repulsion_loss on the GPU.  The distance order is pinned, so
the kernel's indices and distance bits must EQUAL the numpy restatement of
tests/knn_restated.py -- no margins; the repulsion gradient is held to the
float32 summation bound derived there, over the kernel's own (exact) lists."""
import numpy as np
import pytest
import torch

import knn_restated as R

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 20, 32]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _cloud(seed, b, n):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g)


def _assert_exact(query, ref, k, cuda, rows=None, variant=None, msg="", want=None):
    """knn_points (or the forced variant) equals the restatement bit for bit.
    want: the restatement's (dist, idx) for a k at least this one, computed once
    and shared: a list is a prefix of every longer list of the same inputs."""
    import knn
    import pcm_hip
    q, r = query.to(cuda), ref.to(cuda)
    if variant is None:
        dist, idx = knn.knn_points(q, r, k)
    else:
        dist = torch.empty(q.shape[0], q.shape[1], k, device=cuda)
        idx = torch.empty(q.shape[0], q.shape[1], k, dtype=torch.int32, device=cuda)
        pcm_hip.knn(q, 0, r, 0, k, dist, idx, variant=variant)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32
    assert tuple(dist.shape) == tuple(idx.shape) == (query.shape[0], query.shape[1], k)
    assert not dist.requires_grad
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    if rows is not None:
        dist, idx = dist[:, rows], idx[:, rows]
    if want is None:
        want = R.knn_restated(query.numpy(), ref.numpy(), k, rows=rows)
    want_d, want_i = want[0][:, :, :k], want[1][:, :, :k]
    np.testing.assert_array_equal(idx, want_i, err_msg=f"{msg} k={k}")
    np.testing.assert_array_equal(_bits(dist), _bits(want_d), err_msg=f"{msg} k={k}")


def _assert_exact_ks(query, ref, ks, cuda, variant=None, msg=""):
    """_assert_exact for every k of ks against one restatement at the largest."""
    want = R.knn_restated(query.numpy(), ref.numpy(), max(ks))
    for k in ks:
        _assert_exact(query, ref, k, cuda, variant=variant, msg=msg, want=want)


@pytest.mark.parametrize("n,m", [(1, 1), (3, 2), (64, 64), (65, 63), (257, 255), (300, 1025)])
def test_equals_the_restatement(cuda, n, m):
    query, ref = _cloud(10 + n, 2, n), _cloud(20 + m, 2, m)
    _assert_exact_ks(query, ref, KS, cuda, msg=f"n={n} m={m}")


def _boundary_sizes():
    """(n, m) on either side of every boundary the dispatcher has: the 64
    queries of a workgroup, the reference tile, the four candidates of one LDS
    read (the tile is padded to them; with the cloud split over four waves a wave's
    share is a multiple of them and its quarter of the tile a fourth of KNN_TILE)."""
    import pcm_hip
    q, t = pcm_hip.KNN_QUERIES, pcm_hip.KNN_TILE
    ns = [q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1]
    ms = [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17, t - 1, t, t + 1, t + 3, t + 4, t + 5, 2 * t - 1, 2 * t,
          2 * t + 1]
    return [(n, 40 + 3 * i) for i, n in enumerate(ns)] + [(33 + i, m) for i, m in enumerate(ms)]


def test_boundary_sizes_and_every_list_width(cuda):
    import pcm_hip
    sizes = _boundary_sizes()
    assert len(sizes) <= 40
    # k on either side of every list width, so each width meets each boundary
    ks = sorted({1, pcm_hip.KNN_MAX_K} | {w for w in pcm_hip.KNN_WIDTHS} | {w + 1 for w in pcm_hip.KNN_WIDTHS[:-1]})
    assert ks == [1, 4, 5, 8, 9, 16, 17, 20, 21, 32]
    for s, (n, m) in enumerate(sizes):
        query, ref = _cloud(300 + s, 1, n), _cloud(400 + s, 1, m)
        want = R.knn_restated(query.numpy(), ref.numpy(), pcm_hip.KNN_MAX_K)
        for k in KS:  # the named list, on the form the library picks
            _assert_exact(query, ref, k, cuda, msg=f"n={n} m={m}", want=want)
        for v, variant in enumerate((None, 2, 3)):  # the library's pick, one wave, four waves
            for k in (ks[(s + v) % len(ks)], ks[(s + v + 3) % len(ks)]):
                _assert_exact(query, ref, k, cuda, variant=variant, msg=f"n={n} m={m} variant={variant}", want=want)


def test_either_side_of_the_split_dispatch(cuda):
    import pcm_hip
    # the grid size at which pcm_knn stops splitting the reference cloud over four waves
    b = 1
    while pcm_hip.knn_default_split(b + 1, 64) == pcm_hip.KNN_SPLIT:
        b += 1
    assert pcm_hip.knn_default_split(b, 64) == pcm_hip.KNN_SPLIT and pcm_hip.knn_default_split(b + 1, 64) == 1
    query, ref = _cloud(35, b + 1, 64), _cloud(36, b + 1, 30)
    want = R.knn_restated(query.numpy(), ref.numpy(), max(KS))
    for k in KS:
        _assert_exact(query, ref, k, cuda, msg="one wave", want=want)
        _assert_exact(query[:b], ref[:b], k, cuda, msg="split", want=(want[0][:b], want[1][:b]))


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_every_kernel_form_agrees_with_the_restatement(cuda, variant):
    query, ref = _cloud(31, 2, 130), _cloud(32, 2, 1100)
    for k in (3, 8, 20, 32):
        _assert_exact(query, ref, k, cuda, variant=variant, msg=f"variant {variant}")


def test_ties_go_to_the_lower_index(cuda):
    import knn
    # a duplicated cloud: every distance appears twice
    half = _cloud(41, 2, 150)
    dup = torch.cat([half, half], dim=1)
    for k in KS:
        _assert_exact(dup, dup, k, cuda, msg="duplicated")
    dist, idx = knn.knn_points(dup.to(cuda), dup.to(cuda), 2)
    want = torch.arange(150).repeat(2).view(1, 300, 1) + torch.tensor([0, 150]).view(1, 1, 2)
    assert torch.equal(idx.cpu().long(), want.expand(2, 300, 2))  # itself and its copy, the lower index first
    assert (dist == 0).all()
    # a coarse lattice: many equal distances, all exactly representable
    g = torch.Generator().manual_seed(42)
    lattice = torch.randint(0, 4, (2, 400, 3), generator=g).float() * 0.25
    for k in KS:
        _assert_exact(lattice, lattice, k, cuda, msg="lattice")
        _assert_exact(lattice[:, :77], lattice, k, cuda, msg="lattice rows")


def test_non_finite_points_and_queries_follow_the_slot_rule(cuda):
    import knn
    ref = _cloud(51, 2, 90)
    query = _cloud(52, 2, 70)
    ref[0, 3, 1] = float("nan")
    ref[0, 17, 0] = float("inf")
    ref[1, 5, 2] = float("-inf")
    ref[1, 80] = float("nan")
    ref[0, 40, 0] = 3e19  # every distance to it overflows to +inf
    query[0, 2, 0] = float("nan")
    query[1, 9, 1] = float("inf")
    query[1, 64, 2] = float("-inf")
    for k in KS:
        _assert_exact(query, ref, k, cuda, msg="non-finite")
        _assert_exact(ref, ref, k, cuda, msg="non-finite self")
    dist, idx = knn.knn_points(query.to(cuda), ref.to(cuda), 5)
    for bi, i in ((0, 2), (1, 9), (1, 64)):  # a non-finite query lists nothing
        assert (idx[bi, i] == -1).all() and torch.isinf(dist[bi, i]).all() and (dist[bi, i] > 0).all()
    assert not (idx[0] == 3).any() and not (idx[0] == 17).any() and not (idx[0] == 40).any()
    assert not (idx[1] == 5).any() and not (idx[1] == 80).any()
    assert not torch.isnan(dist).any()
    # only non-finite candidates: every slot is empty; fewer candidates than k: the tail is
    bad = torch.full((1, 6, 3), float("nan"))
    dist, idx = knn.knn_points(query[:1].to(cuda), bad.to(cuda), 3)
    assert (idx == -1).all() and torch.isinf(dist).all()
    dist, idx = knn.knn_points(query[:1].to(cuda), ref[:1, 50:52].to(cuda), 5)
    assert (idx[0, 0, :2] >= 0).all() and (idx[0, 0, 2:] == -1).all() and torch.isinf(dist[0, 0, 2:]).all()


def test_subnormal_distances_keep_their_bits(cuda):
    # coordinates near 1e-20: every squared distance is a float32 subnormal (or zero), which the
    # distance, the sorted insert and the merge must carry unchanged
    query, ref = _cloud(55, 2, 70) * 1e-20, _cloud(56, 2, 1100) * 1e-20
    want_d, _ = R.knn_restated(query.numpy(), ref.numpy(), 32)
    tiny = np.float32(2.0 ** -126)
    assert (want_d < tiny).all() and (want_d > 0).sum() > want_d.size // 2
    for variant in (None, 1, 2, 3):
        _assert_exact_ks(query, ref, KS, cuda, variant=variant, msg=f"subnormal variant={variant}")
    # the same scale with ties: a lattice whose steps are subnormal once squared
    g = torch.Generator().manual_seed(57)
    lattice = torch.randint(0, 4, (1, 300, 3), generator=g).float() * 1e-20
    for k in KS:
        _assert_exact(lattice, lattice, k, cuda, msg="subnormal lattice")


def test_many_small_clouds_and_one_alone(cuda):
    import knn
    b, n, m = 300, 40, 50
    query, ref = _cloud(61, b, n), _cloud(62, b, m)
    _assert_exact_ks(query, ref, KS, cuda, msg="b=300")
    dist, idx = knn.knn_points(query.to(cuda), ref.to(cuda), 5)
    alone_d, alone_i = knn.knn_points(query[b - 1:].to(cuda), ref[b - 1:].to(cuda), 5)
    assert torch.equal(alone_i, idx[b - 1:]) and torch.equal(alone_d.view(torch.int32), dist[b - 1:].view(torch.int32))


def test_largest_case_and_one_past_it(cuda):
    import knn
    import pcm_hip
    n, k = pcm_hip.KNN_MAX_POINTS, pcm_hip.KNN_MAX_K
    cloud = _cloud(71, 1, n)
    rows = np.sort(np.random.default_rng(72).choice(n, 256, replace=False))
    _assert_exact(cloud, cloud, k, cuda, rows=rows, msg="largest")
    # one point more, on either side, is rejected on the host: nothing is launched, the outputs stay
    big = torch.zeros(1, n + 1, 3, device=cuda)
    small = torch.zeros(1, 8, 3, device=cuda)
    for q, r in ((big, small), (small, big)):
        dist = torch.full((1, q.shape[1], 2), -7.0, device=cuda)
        idx = torch.full((1, q.shape[1], 2), -7, dtype=torch.int32, device=cuda)
        with pytest.raises(pcm_hip.PcmError):
            pcm_hip.knn(q, 0, r, 0, 2, dist, idx)
        with pytest.raises(pcm_hip.PcmError):
            knn.knn_points(q, r, 2)
        torch.cuda.synchronize()
        assert (dist == -7).all() and (idx == -7).all()
    dist = torch.full((1, 8, k + 1), -7.0, device=cuda)
    idx = torch.full((1, 8, k + 1), -7, dtype=torch.int32, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.knn(small, 0, small, 0, k + 1, dist, idx)
    torch.cuda.synchronize()
    assert (dist == -7).all() and (idx == -7).all()


def test_k1_is_the_chamfer_forward(cuda):
    import dist_chamfer_3D
    import knn
    for n, m in ((300, 1025), (1024, 1024)):
        x1, x2 = _cloud(81, 2, n).to(cuda), _cloud(82, 2, m).to(cuda)
        d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DDist()(x1, x2)
        dist, idx = knn.knn_points(x1, x2, 1)
        assert torch.equal(idx[:, :, 0], i1.int()) and torch.equal(dist[:, :, 0].contiguous().view(torch.int32),
                                                                  d1.contiguous().view(torch.int32))
        dist, idx = knn.knn_points(x2, x1, 1)
        assert torch.equal(idx[:, :, 0], i2.int()) and torch.equal(dist[:, :, 0].contiguous().view(torch.int32),
                                                                  d2.contiguous().view(torch.int32))


def test_planes_views_equal_rows_and_the_module_convention(cuda):
    import knn
    import pcm_hip
    query, ref = _cloud(91, 2, 130).to(cuda), _cloud(92, 2, 300).to(cuda)
    rows_d, rows_i = knn.knn_points(query, ref, 7)
    qp = query.transpose(1, 2).contiguous()  # [B, 3, N]
    rp = ref.transpose(1, 2).contiguous()
    assert pcm_hip.cloud_layout(qp.transpose(1, 2)) == 1
    for q, r in ((qp.transpose(1, 2), ref), (query, rp.transpose(1, 2)), (qp.transpose(1, 2), rp.transpose(1, 2))):
        d, i = knn.knn_points(q, r, 7)
        assert torch.equal(i, rows_i) and torch.equal(d.view(torch.int32), rows_d.view(torch.int32))
    # any other stride is made contiguous first
    wide = torch.zeros(2, 130, 4, device=cuda)
    wide[:, :, :3] = query
    d, i = knn.knn_points(wide[:, :, :3], ref, 7)
    assert torch.equal(i, rows_i)
    # KNN(k, transpose_mode)(ref, query): Euclidean distances, int64 indices
    d, i = knn.KNN(k=7, transpose_mode=True)(ref, query)
    assert i.dtype == torch.int64 and tuple(d.shape) == (2, 130, 7) and not d.requires_grad
    assert torch.equal(i, rows_i.long()) and torch.equal(d, torch.sqrt(rows_d))
    d, i = knn.KNN(k=7)(rp, qp)
    assert tuple(d.shape) == tuple(i.shape) == (2, 7, 130) and d.is_contiguous()
    assert torch.equal(i, rows_i.long().transpose(1, 2)) and torch.equal(d, torch.sqrt(rows_d).transpose(1, 2))
    d, i = knn.KNN(k=7, transpose_mode=True)(ref, query.clone().requires_grad_(True))
    assert not d.requires_grad


def test_side_stream_and_graph_replay_equal_eager(cuda):
    import knn
    import pcm_hip
    first_q, first_r = _cloud(101, 2, 200), _cloud(102, 2, 1500)
    second_q, second_r = _cloud(103, 2, 200), _cloud(104, 2, 1500)
    k = 20
    eager = knn.knn_points(first_q.to(cuda), first_r.to(cuda), k)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = knn.knn_points(first_q.to(cuda), first_r.to(cuda), k)
    side.synchronize()
    assert torch.equal(eager[1], other[1]) and torch.equal(eager[0].view(torch.int32), other[0].view(torch.int32))

    sq, sr = first_q.to(cuda).clone(), first_r.to(cuda).clone()
    dist = torch.empty(2, 200, k, device=cuda)
    idx = torch.empty(2, 200, k, dtype=torch.int32, device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pcm_hip.knn(sq, 0, sr, 0, k, dist, idx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm_hip.knn(sq, 0, sr, 0, k, dist, idx)
    for q, r in ((second_q, second_r), (first_q, first_r)):
        sq.copy_(q.to(cuda))
        sr.copy_(r.to(cuda))
        idx.fill_(-5)
        graph.replay()
        torch.cuda.synchronize()
        want_d, want_i = R.knn_restated(q.numpy(), r.numpy(), k)
        np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
        np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want_d))


def test_properties_that_do_not_rest_on_the_restatement(cuda):
    import knn
    b, n, m, k = 2, 150, 700, 20
    query, ref = _cloud(111, b, n), _cloud(112, b, m)
    dist, idx = knn.knn_points(query.to(cuda), ref.to(cuda), k)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    assert (dist[:, :, 1:] >= dist[:, :, :-1]).all()  # every list ascends
    assert (idx >= 0).all() and (idx < m).all()
    d64 = ((ref.numpy().astype(np.float64)[:, None] - query.numpy().astype(np.float64)[:, :, None]) ** 2).sum(-1)
    for bi in range(b):
        for i in range(n):
            assert len(set(idx[bi, i].tolist())) == k
            unlisted = np.delete(d64[bi, i], idx[bi, i])
            kth = d64[bi, i, idx[bi, i, k - 1]]
            assert unlisted.min() >= kth * (1 - 1e-5), (bi, i)


# ---------------------------------------------------------------------------
# repulsion loss
# ---------------------------------------------------------------------------

REPULSION_SHAPES = [(2, 64, 0.02), (3, 300, 0.01), (2, 1024, 0.004), (2, 1024, 0.0005)]
_restated = {}


def _repulsion_case(b, n, h):
    """A uniform cloud and the restatement's loss, share and lists: computed once, never changed."""
    key = (b, n, h)
    if key not in _restated:
        xyz = _cloud(500 + n, b, n)
        _restated[key] = (xyz,) + R.repulsion_restated(xyz.numpy(), h)
    return _restated[key]


def _run_repulsion(xyz_dev, lay, h, want_grad=True):
    import pcm_hip
    loss = torch.full((1,), -7.0, device=xyz_dev.device)
    grad = None
    if want_grad:
        grad = torch.full_like(xyz_dev, -7.0) if lay == 0 else \
            torch.full_like(xyz_dev.transpose(1, 2), -7.0).transpose(1, 2)
    pcm_hip.repulsion_loss(xyz_dev, lay, h, loss, grad)
    return loss, grad


@pytest.mark.parametrize("b,n,h", REPULSION_SHAPES)
def test_repulsion_loss_and_gradient(cuda, b, n, h):
    import knn
    xyz, want_loss, share, want_d, want_i = _repulsion_case(b, n, h)
    if h == 0.0005:
        assert share > 0  # the default h: about 1.5 % of the terms
    else:
        assert 0.1 < share < 0.9
    dev = xyz.to(cuda)
    loss, grad = _run_repulsion(dev, 0, h)
    print(f"repulsion b={b} n={n} h={h}: active share {share:.4f} loss {loss.item():.9g} restated {want_loss:.9g}")
    np.testing.assert_allclose(loss.item(), want_loss, rtol=2e-6, atol=0)
    # the loss alone: the same bits
    alone, _ = _run_repulsion(dev, 0, h, want_grad=False)
    assert torch.equal(alone.view(torch.int32), loss.view(torch.int32))
    # the kernel's own lists are the restatement's (proven exact above), and the gradient is held to the
    # float32 summation bound over them
    dist, idx = knn.knn_points(dev, dev, 5)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(_bits(dist.cpu().numpy()), _bits(want_d))
    ref, count, mag = R.repulsion_gradient_f64(xyz.numpy(), dist.cpu().numpy(), idx.cpu().numpy(), h)
    bound = R.gradient_bound(count, mag)
    got = grad.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"  gradient: largest error / bound {worst:.3f}; points with terms {int((count > 0).sum())}")
    assert (err <= bound).all()
    assert (got[count == 0] == 0).all()
    assert np.abs(ref).max() > 0
    # every cloud's gradient sums to zero within the same bound
    assert (np.abs(got.sum(1)) <= bound.sum(1)).all()
    # two calls give identical bits
    loss2, grad2 = _run_repulsion(dev, 0, h)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32))
    # the planes view: the same bits, the gradient in planes
    planes = dev.transpose(1, 2).contiguous().transpose(1, 2)
    loss3, grad3 = _run_repulsion(planes, 1, h)
    assert grad3.transpose(1, 2).is_contiguous()
    assert torch.equal(loss3.view(torch.int32), loss.view(torch.int32))
    assert torch.equal(grad3.contiguous().view(torch.int32), grad.view(torch.int32))


def test_repulsion_h_zero_and_duplicates(cuda):
    xyz = _cloud(121, 2, 200)
    loss, grad = _run_repulsion(xyz.to(cuda), 0, 0.0)
    assert loss.item() == 0 and (grad == 0).all()
    # a duplicated cloud: slot 0 and slot 1 are the point and its copy at distance 0, so one slot of
    # every point adds exactly h and no gradient; with h below every other distance nothing else is active
    dup = torch.cat([xyz, xyz], dim=1)
    d = R.knn_restated(xyz.numpy(), xyz.numpy(), 2)[0][:, :, 1]
    h = float(np.float32(d.min() / 2))
    assert h > 0
    loss, grad = _run_repulsion(dup.to(cuda), 0, h)
    np.testing.assert_allclose(loss.item(), h / 4, rtol=2e-6, atol=0)
    assert (grad == 0).all()


def test_repulsion_graph_replay_equals_eager(cuda):
    import pcm_hip
    b, n, h = 2, 300, 0.01
    first, second = _cloud(131, b, n), _cloud(132, b, n)
    eager = {}
    for name, c in (("first", first), ("second", second)):
        eager[name] = _run_repulsion(c.to(cuda), 0, h)
    torch.cuda.synchronize()
    static = first.to(cuda).clone()
    loss = torch.empty(1, device=cuda)
    grad = torch.empty_like(static)
    ws = torch.empty(int(pcm_hip.load_library().pcm_repulsion_workspace_bytes(b, n)), dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pcm_hip.repulsion_loss(static, 0, h, loss, grad, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm_hip.repulsion_loss(static, 0, h, loss, grad, workspace=ws)
    for name, c in (("second", second), ("first", first)):
        static.copy_(c.to(cuda))
        grad.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.view(torch.int32), eager[name][0].view(torch.int32))
        assert torch.equal(grad.view(torch.int32), eager[name][1].view(torch.int32))
    # a workspace one byte short is refused
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.repulsion_loss(static, 0, h, loss, grad, workspace=ws[:-1])


def test_loss_class_backpropagates_into_the_generator_layout(cuda):
    import loss as loss_mod
    b, n = 2, 300
    xyz = _cloud(141, b, n)
    h = 0.01
    gen_out = xyz.transpose(1, 2).contiguous().to(cuda).requires_grad_(True)  # [B, 3, N]
    value = loss_mod.Loss().get_repulsion_loss(gen_out.transpose(2, 1), h=h)
    assert value.dim() == 0 and value.requires_grad
    (value * 3.0).backward()
    assert tuple(gen_out.grad.shape) == (b, 3, n) and gen_out.grad.is_contiguous()
    want_loss, want_grad = _run_repulsion(xyz.to(cuda), 0, h)
    assert torch.equal(value.detach().view(1).view(torch.int32), want_loss.view(torch.int32))
    assert torch.equal(gen_out.grad.transpose(1, 2), 3.0 * want_grad)
    assert (gen_out.grad != 0).any()
    # rows, and the default h
    rows = xyz.to(cuda).requires_grad_(True)
    loss_mod.Loss().get_repulsion_loss(rows, h=h).backward()
    assert torch.equal(rows.grad, want_grad)
    default = loss_mod.Loss().get_repulsion_loss(xyz.to(cuda))
    assert not default.requires_grad and default.item() >= 0
    # an empty batch: the mean over nothing (NaN, as torch.mean's) and an empty gradient
    empty = torch.empty(0, n, 3, device=cuda, requires_grad=True)
    value = loss_mod.Loss().get_repulsion_loss(empty, h=h)
    assert torch.isnan(value).item()
    value.backward()
    assert tuple(empty.grad.shape) == (0, n, 3)
    assert torch.isnan(loss_mod.Loss().get_repulsion_loss(empty.detach(), h=h)).item()
