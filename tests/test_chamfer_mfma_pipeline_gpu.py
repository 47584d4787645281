"""The pipelined screen loop of the one-launch Chamfer step's matrix-core
forward (fused variants 6 and 19, csrc/chamfer_filt.hip filt_forward_mfma).

The loop folds an MFMA's result three MFMAs later, over four rotating result
quads, carries a group's last folds and its best/second/chunk update into the
next group's first gaps, and re-reads each A tile in place for the wave's next
group.  Every case compares the forward (distances, argmins) and the gradients
bit for bit with the CPU oracle.  In a launch with clouds of n and m points,
direction 1 screens n queries against m targets and direction 2 the reverse;
a wave (quarter q of a workgroup) screens the 64-target groups q, q + 4, ...
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MFMA_VARIANTS = (6, 19)  # counter hand-off, granule hand-off


def _outputs(cuda, b, n, m, planes1=False, planes2=False):
    def grad(k, planes):
        if planes:
            return torch.full((b, 3, k), float("nan"), device=cuda).transpose(1, 2)
        return torch.full((b, k, 3), float("nan"), device=cuda)
    return (torch.empty(b, n, device=cuda), torch.empty(b, m, device=cuda),
            torch.full((b, n), -1, dtype=torch.int32, device=cuda),
            torch.full((b, m), -1, dtype=torch.int32, device=cuda),
            torch.full((3,), float("nan"), device=cuda), grad(n, planes1), grad(m, planes2))


def _reference(oracle, a, c):
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    an, cn = a.numpy(), c.numpy()
    r1, r2, j1, j2 = oracle.chamfer_forward(an, cn)
    w1, w2 = np.float32(1.0 / (b * n)), np.float32(1.0 / (b * m))
    gr1, gr2 = oracle.chamfer_backward(an, cn, np.full((b, n), w1, np.float32), np.full((b, m), w2, np.float32),
                                       j1, j2)
    return (r1, r2, j1, j2, gr1, gr2), (w1, w2)


def _assert_equal(out, ref, what):
    d1, d2, i1, i2, _, g1, g2 = out
    r1, r2, j1, j2, gr1, gr2 = ref
    np.testing.assert_array_equal(i1.cpu().numpy(), j1, err_msg=what)
    np.testing.assert_array_equal(i2.cpu().numpy(), j2, err_msg=what)
    np.testing.assert_array_equal(d1.cpu().numpy().view(np.int32), r1.view(np.int32), err_msg=what)
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.int32), r2.view(np.int32), err_msg=what)
    np.testing.assert_array_equal(g1.cpu().contiguous().numpy().view(np.int32), gr1.view(np.int32), err_msg=what)
    np.testing.assert_array_equal(g2.cpu().contiguous().numpy().view(np.int32), gr2.view(np.int32), err_msg=what)


def _check(cuda, oracle, a, c):
    """Both matrix-core variants on row clouds; returns variant 19's argmins of direction 1."""
    import pcm_hip
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    ref, (w1, w2) = _reference(oracle, a, c)
    x1, x2 = a.to(cuda), c.to(cuda)
    for v in MFMA_VARIANTS:
        out = _outputs(cuda, b, n, m)
        pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, variant=v)
        torch.cuda.synchronize()
        _assert_equal(out, ref, f"variant {v}, n={n}, m={m}")
    return out[2].cpu().numpy()


def _clouds(seed, b, n, m):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g), torch.rand(b, m, 3, generator=g)


@pytest.mark.parametrize("nt", [128, 129, 192, 256, 257, 320, 448, 512, 513, 576, 768, 832, 960, 961])
def test_mfma_pipeline_group_counts(cuda, oracle, nt):
    # 2..16 target groups: a wave runs 0, 1, 2, 3 or 4 of them (odd and even
    # counts), its last group re-reads itself, and the last group of the cloud
    # is part padding where nt is no multiple of 64; the folds and the update
    # that cross from one group into the next run once per further group
    for nq in (64, 257):
        a, c = _clouds(3000 * nt + nq, 2, nq, nt)
        _check(cuda, oracle, a, c)


def test_mfma_pipeline_winner_in_every_position(cuda, oracle):
    # batch element r: query k sits 1e-4 from target 4 k + r, so over the four
    # elements every target -- every (group, tile, result quad, lane group, row)
    # of the screen -- is the argmin of some query
    b, nq, nt = 4, 256, 1024
    g = torch.Generator().manual_seed(4242)
    c = torch.rand(b, nt, 3, generator=g)
    off = (torch.rand(b, nq, 3, generator=g) * 2.0 - 1.0) * 1e-4
    want = 4 * np.arange(nq)[None, :] + np.arange(b)[:, None]
    a = torch.stack([c[r, want[r]] for r in range(b)]) + off
    i1 = _check(cuda, oracle, a, c)
    np.testing.assert_array_equal(i1, want.astype(np.int32))


@pytest.mark.parametrize("lays", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_mfma_pipeline_layout_instances(cuda, oracle, lays):
    # the default variant's four layout instances (rows or channel planes per
    # cloud), each its own instantiation of the loop, at an odd size
    import pcm_hip
    b, n, m = 2, 257, 193
    a, c = _clouds(77, b, n, m)
    ref, (w1, w2) = _reference(oracle, a, c)
    x1 = a.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[0] else a.to(cuda)
    x2 = c.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[1] else c.to(cuda)
    assert (pcm_hip.cloud_layout(x1), pcm_hip.cloud_layout(x2)) == lays
    out = _outputs(cuda, b, n, m, planes1=bool(lays[0]), planes2=bool(lays[1]))
    pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, layouts=lays)
    torch.cuda.synchronize()
    _assert_equal(out, ref, f"layouts {lays}")
