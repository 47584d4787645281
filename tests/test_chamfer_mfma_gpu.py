"""The matrix-core screen of the one-launch Chamfer step (fused variants 6 and
19, csrc/chamfer_filt.hip filt_forward_mfma) at the edges of its geometry.

Every case compares the forward (distances, argmins) and the gradients bit for
bit with the CPU oracle.  In a launch with clouds of n and m points, direction
1 screens n queries against m targets and direction 2 the reverse.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MFMA_VARIANTS = (6, 19)  # counter hand-off, granule hand-off


def _check(cuda, oracle, a, c):
    import pcm_hip
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    an, cn = a.numpy(), c.numpy()
    r1, r2, j1, j2 = oracle.chamfer_forward(an, cn)
    w1, w2 = np.float32(1.0 / (b * n)), np.float32(1.0 / (b * m))
    gr1, gr2 = oracle.chamfer_backward(an, cn, np.full((b, n), w1, np.float32), np.full((b, m), w2, np.float32),
                                       j1, j2)
    x1, x2 = a.to(cuda), c.to(cuda)
    for v in MFMA_VARIANTS:
        d1, d2 = torch.empty(b, n, device=cuda), torch.empty(b, m, device=cuda)
        i1 = torch.full((b, n), -1, dtype=torch.int32, device=cuda)
        i2 = torch.full((b, m), -1, dtype=torch.int32, device=cuda)
        g1 = torch.full((b, n, 3), float("nan"), device=cuda)
        g2 = torch.full((b, m, 3), float("nan"), device=cuda)
        mo = torch.full((3,), float("nan"), device=cuda)
        pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, d1, d2, i1, i2, mo, g1, g2, variant=v)
        torch.cuda.synchronize()
        what = f"variant {v}, n={n}, m={m}"
        np.testing.assert_array_equal(i1.cpu().numpy(), j1, err_msg=what)
        np.testing.assert_array_equal(i2.cpu().numpy(), j2, err_msg=what)
        np.testing.assert_array_equal(d1.cpu().numpy().view(np.int32), r1.view(np.int32), err_msg=what)
        np.testing.assert_array_equal(d2.cpu().numpy().view(np.int32), r2.view(np.int32), err_msg=what)
        np.testing.assert_array_equal(g1.cpu().numpy().view(np.int32), gr1.view(np.int32), err_msg=what)
        np.testing.assert_array_equal(g2.cpu().numpy().view(np.int32), gr2.view(np.int32), err_msg=what)


def _clouds(seed, b, n, m):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g), torch.rand(b, m, 3, generator=g)


@pytest.mark.parametrize("nt", [1, 15, 16, 17, 63, 64, 65, 1023, 1024])
def test_mfma_screen_edge_sizes(cuda, oracle, nt):
    # pad rows inside a 16-row tile and a 64-target group, partial groups per
    # quarter, one workgroup and a part-filled second one
    for nq in (1, 255, 256, 257):
        a, c = _clouds(1000 * nt + nq, 2, nq, nt)
        _check(cuda, oracle, a, c)


def test_mfma_screen_subnormal_parts(cuda, oracle):
    # the lower bf16 parts of the split, w and every product go subnormal or to
    # zero: only the bound's absolute 2^-100 term covers the screen's error
    a, c = _clouds(7, 2, 300, 500)
    _check(cuda, oracle, a * 1e-30, c * 1e-30)


def test_mfma_screen_w_overflow(cuda, oracle):
    # finite inputs whose centred squared norms overflow: w = +inf, NaN parts
    a, c = _clouds(8, 2, 300, 500)
    _check(cuda, oracle, a * 3e19, c * 3e19)


def _listed_near_ties(q, t):
    """Float64 restatement of the screen's proof for one workgroup (its <= 256
    queries q against the targets t): how many queries it lists as near ties.
    A chunk is one lane group of one 64-target group: target k lies in chunk
    4 (k >> 6) + ((k & 15) >> 2)."""
    q, t = q.astype(np.float64), t.astype(np.float64)
    c = q.mean(axis=0)
    qc, tc = q - c, t - c
    w = (tc * tc).sum(axis=1)
    a = w[None, :] - 2.0 * qc @ tc.T
    k = np.arange(t.shape[0])
    chunk = 4 * (k >> 6) + ((k & 15) >> 2)
    mins = np.full((q.shape[0], chunk.max() + 1), np.inf)
    for ch in np.unique(chunk):
        mins[:, ch] = a[:, chunk == ch].min(axis=1)
    srt = np.sort(mins, axis=1)
    fb, fs = srt[:, 0], (srt[:, 1] if srt.shape[1] > 1 else np.full(q.shape[0], np.inf))
    u80, kabs = 80.0 * 2.0 ** -24, 2.0 ** -100
    qn2 = (qc * qc).sum(axis=1)
    sq = np.sqrt(qn2)
    rr = np.sqrt(w.max()) + sq
    e_r = u80 * rr * rr * 1.001 + kabs
    db = np.maximum((fb + qn2) * 1.0001 + 2.0 * e_r, 0.0)
    rq = 2.0 * sq + np.sqrt(db)
    e2 = 2.0 * (u80 * np.minimum(rr * rr, rq * rq) * 1.001 + kabs)
    return int((~((fs - fb) > e2)).sum())


def test_mfma_screen_many_near_ties(cuda, oracle):
    # every target has a twin 1e-7 away in ANOTHER chunk (four targets on: the
    # next lane group of the same tile), so the best chunk always has a rival
    # inside the bound: more listed queries than the workgroup has waves, and
    # the near-tie pass runs several rounds
    a, c = _clouds(9, 2, 256, 64)
    for base in range(0, 64, 8):
        c[:, base + 4:base + 8] = c[:, base:base + 4] + 1e-7
    for e in range(2):  # direction 1: one 256-query workgroup per batch element
        assert _listed_near_ties(a[e].numpy(), c[e].numpy()) > 8
    _check(cuda, oracle, a, c)
