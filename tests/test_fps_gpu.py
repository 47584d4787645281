"""pcm_fps on the GPU: exact equality with the reference's indices where the
fixture reaches, elsewhere with a numpy restatement of include/pcm.h's
contract on clouds whose every used pick is decided by a relative margin of
at least 1e-6 (about 8 float32 ulps) or by an exact tie -- asserted first, so
that equality is a fair demand whatever order a correctly rounded distance is
summed in -- and two properties that do not rest on the restatement at all."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "fps_golden.npz")
MARGIN = 1e-6


def _sqd_pinned(d):
    # fmaf(dz, dz, fmaf(dy, dy, dx * dx)): each fused step formed in float64
    # (the product is exact there) and rounded once
    dx, dy, dz = (d[:, c].astype(np.float32) for c in range(3))
    t = (dx * dx).astype(np.float32)
    t = (dy.astype(np.float64) * dy + t).astype(np.float32)
    return (dz.astype(np.float64) * dz + t).astype(np.float32)


def fps_restated(xyz, npoint, start):
    """include/pcm.h's contract of pcm_fps in numpy: idx [B, npoint] int64 and
    the smallest relative margin by which a used pick's winner beats the next
    distinct running minimum (exact ties aside; inf if there is none)."""
    b, n, _ = xyz.shape
    idx = np.zeros((b, npoint), np.int64)
    worst = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(b):
            p = xyz[bi]
            run = np.full(n, 1e10, np.float32)
            far = start
            for i in range(npoint):
                idx[bi, i] = far
                d = _sqd_pinned(p - p[far])
                upd = d < run
                run[upd] = d[upd]
                far = int(np.argmax(run))
                if i + 1 < npoint:
                    v1 = run[far]
                    below = run[run != v1]
                    if below.size:
                        worst = min(worst, float((np.float64(v1) - below.max()) / v1))
    return idx, worst


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {name: (z[f"{name}/xyz"], z[f"{name}/idx"], int(z[f"{name}/npoint"]), bool(z[f"{name}/ran"]))
            for name in z["cases"]}


CASES = ["train128", "train256", "ragged", "odd", "two_chunks", "dups", "tiny", "oversample", "nonfinite"]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _cloud(seed, b, n):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g)


def _checked(seed, b, n, s, start=0):
    """A seeded cloud and the restatement's indices, the margin asserted."""
    xyz = _cloud(seed, b, n)
    want, worst = fps_restated(xyz.numpy(), s, start)
    assert worst >= MARGIN, f"seed {seed}: a pick of the test's own cloud is decided by {worst:.3g}"
    return xyz, want


@pytest.mark.parametrize("name", CASES)
def test_fixture_indices_and_sampled_points(cuda, golden, name):
    import sampling
    xyz_np, idx_np, s, ran = golden[name]
    xyz = torch.from_numpy(xyz_np).to(cuda)
    idx = sampling.farthest_point_sample(xyz, s, RAN=ran)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == idx_np.shape and idx.device == xyz.device
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_np)
    idx2, new_xyz = sampling.sample_points(xyz, s, RAN=ran)
    np.testing.assert_array_equal(idx2.cpu().numpy(), idx_np)
    assert new_xyz.dtype == torch.float32 and tuple(new_xyz.shape) == idx_np.shape + (3,)
    assert not new_xyz.requires_grad
    gathered = sampling.index_points(xyz, torch.from_numpy(idx_np).to(cuda))
    assert _same_bits(new_xyz, gathered)  # bit for bit, the NaN and the infinities included


def test_planes_view_is_read_in_place(cuda, golden):
    import pcm_hip
    import sampling
    xyz_np, idx_np, s, ran = golden["ragged"]
    planes = torch.from_numpy(xyz_np).to(cuda).transpose(1, 2).contiguous()  # [B, 3, N]
    view = planes.transpose(1, 2)
    assert pcm_hip.cloud_layout(view) == 1
    idx, new_xyz = sampling.sample_points(view, s, RAN=ran)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_np)
    assert _same_bits(new_xyz, sampling.index_points(view, idx))
    # any other stride is made contiguous first
    wide = torch.zeros(xyz_np.shape[0], xyz_np.shape[1], 4, device=cuda)
    wide[:, :, :3] = torch.from_numpy(xyz_np).to(cuda)
    assert pcm_hip.cloud_layout(wide[:, :, :3]) is None
    np.testing.assert_array_equal(sampling.farthest_point_sample(wide[:, :, :3], s, RAN=ran).cpu().numpy(), idx_np)


def _boundary_sizes():
    """Ragged and boundary n: the listed ones, the n on either side of every
    power-of-two capacity of an instance (points per lane double there; 8192 is
    also where the centroid read leaves LDS), and the n on either side of
    every switch of workgroup size the dispatcher makes."""
    import pcm_hip
    sizes = {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025}
    for cap in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        sizes |= {cap, cap + 1}
    prev = pcm_hip.fps_default_threads(1)
    for n in range(2, pcm_hip.FPS_MAX_POINTS + 1):
        t = pcm_hip.fps_default_threads(n)
        if t != prev:
            sizes |= {n - 1, n}
        prev = t
    return sorted(sizes)


def test_ragged_and_boundary_sizes(cuda):
    import pcm_hip
    import sampling
    sizes = _boundary_sizes()
    assert len(sizes) <= 40
    for n in sizes:
        s = min(n, 40)
        xyz, want = _checked(100 + n, 2, n, s)
        idx, new_xyz = sampling.sample_points(xyz.to(cuda), s)
        np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=f"n={n}")
        assert _same_bits(new_xyz.cpu(), sampling.index_points(xyz, torch.from_numpy(want))), n
    assert pcm_hip.FPS_MAX_POINTS not in sizes


def test_largest_cloud_and_one_past_it(cuda):
    import pcm_hip
    import sampling
    n = pcm_hip.FPS_MAX_POINTS
    xyz, want = _checked(7, 1, n, 32)
    idx, new_xyz = sampling.sample_points(xyz.to(cuda), 32)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert _same_bits(new_xyz.cpu(), sampling.index_points(xyz, torch.from_numpy(want)))
    # one point more is rejected on the host: nothing is launched, the outputs stay as they were
    big = torch.zeros(1, n + 1, 3, device=cuda)
    out = torch.full((1, 4), -7, dtype=torch.int64, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.fps(big, 0, 4, 0, out)
    with pytest.raises(pcm_hip.PcmError):
        sampling.farthest_point_sample(big, 4)
    torch.cuda.synchronize()
    assert (out == -7).all()


@pytest.mark.parametrize("b,n,s", [(33, 300, 20), (300, 64, 8)])
def test_batches_above_a_wave_of_workgroups(cuda, b, n, s):
    import sampling
    xyz, want = _checked(1000 + b, b, n, s)
    idx, new_xyz = sampling.sample_points(xyz.to(cuda), s)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert _same_bits(new_xyz.cpu(), sampling.index_points(xyz, torch.from_numpy(want)))
    # a cloud alone gives what it gives in the batch
    alone = sampling.farthest_point_sample(xyz[b - 1:].to(cuda), s)
    np.testing.assert_array_equal(alone.cpu().numpy(), want[b - 1:])


def test_ran_false_starts_every_row_at_one(cuda):
    import sampling
    xyz, want = _checked(31, 4, 130, 20, start=1)
    idx = sampling.farthest_point_sample(xyz.to(cuda), 20, RAN=False)
    assert (idx[:, 0] == 1).all()
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    assert (sampling.farthest_point_sample(xyz.to(cuda), 20)[:, 0] == 0).all()
    with pytest.raises(ValueError):
        sampling.farthest_point_sample(xyz[:, :1].to(cuda), 1, RAN=False)
    one = sampling.farthest_point_sample(xyz[:, :1].to(cuda), 3, RAN=True)
    assert (one == 0).all()


def test_non_default_stream_equals_default_stream(cuda):
    import sampling
    xyz, want = _checked(41, 3, 700, 60)
    dev = xyz.to(cuda)
    default = sampling.sample_points(dev, 60)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = sampling.sample_points(dev, 60)
    side.synchronize()
    np.testing.assert_array_equal(default[0].cpu().numpy(), want)
    assert torch.equal(default[0], other[0]) and _same_bits(default[1], other[1])


def test_graph_replay_equals_eager(cuda):
    import pcm_hip
    first, want_first = _checked(51, 2, 500, 48)
    second, want_second = _checked(52, 2, 500, 48)
    static = first.to(cuda).clone()
    idx = torch.empty(2, 48, dtype=torch.int64, device=cuda)
    new_xyz = torch.empty(2, 48, 3, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pcm_hip.fps(static, 0, 48, 0, idx, new_xyz)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pcm_hip.fps(static, 0, 48, 0, idx, new_xyz)
    import sampling
    for cloud, want in ((second, want_second), (first, want_first)):
        static.copy_(cloud.to(cuda))
        idx.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        assert _same_bits(new_xyz.cpu(), sampling.index_points(cloud, torch.from_numpy(want)))


def test_properties_that_do_not_rest_on_the_restatement(cuda):
    import sampling
    b, n, s = 2, 200, 50
    xyz = _cloud(61, b, n)
    idx = sampling.farthest_point_sample(xyz.to(cuda), s).cpu().numpy()
    p = xyz.numpy().astype(np.float64)
    for bi in range(b):
        picks = idx[bi]
        assert len(set(picks.tolist())) == s  # distinct
        for i in range(1, s):
            # squared distance of every point to its nearest earlier pick
            d = ((p[bi][:, None, :] - p[bi][picks[:i]][None, :, :]) ** 2).sum(-1).min(1)
            assert d[picks[i]] >= d.max() * (1 - 1e-5), (bi, i)


@pytest.mark.parametrize("name", ["ragged", "two_chunks"])
@pytest.mark.parametrize("threads", [64, 256, 1024])
def test_every_forced_workgroup_size_agrees(cuda, golden, name, threads):
    import pcm_hip
    import sampling
    xyz_np, idx_np, s, ran = golden[name]
    xyz = torch.from_numpy(xyz_np).to(cuda)
    b = xyz.shape[0]
    idx = torch.full((b, s), -1, dtype=torch.int64, device=cuda)
    new_xyz = torch.full((b, s, 3), -1.0, device=cuda)
    pcm_hip.fps(xyz, 0, s, 0 if ran else 1, idx, new_xyz, threads=threads)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_np)
    assert _same_bits(new_xyz, sampling.index_points(xyz, idx))
    # and on the channel planes
    planes = xyz.transpose(1, 2).contiguous().transpose(1, 2)
    idx.fill_(-1)
    pcm_hip.fps(planes, 1, s, 0 if ran else 1, idx, None, threads=threads)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx_np)


def test_largest_cloud_on_the_sizes_that_hold_it(cuda):
    # 256 threads hold 64 points a lane; 64 threads do not hold the cloud
    import pcm_hip
    n = pcm_hip.FPS_MAX_POINTS
    xyz, want = _checked(7, 1, n, 32)
    dev = xyz.to(cuda)
    idx = torch.empty(1, 32, dtype=torch.int64, device=cuda)
    for threads in (256, 1024):
        idx.fill_(-1)
        pcm_hip.fps(dev, 0, 32, 0, idx, None, threads=threads)
        np.testing.assert_array_equal(idx.cpu().numpy(), want, err_msg=str(threads))
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.fps(dev, 0, 32, 0, idx, None, threads=64)
