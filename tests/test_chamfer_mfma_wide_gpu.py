"""The wide screen loop of the one-launch Chamfer step's matrix-core forward
(fused variant 20, csrc/chamfer_filt.hip filt_forward_mfma<.., true>): chained
v_mfma_f32_32x32x16_bf16 pairs over 32-row target tiles and 32-query tiles.

A wave (quarter q of a workgroup) screens the 64-target groups q, q + 4, ...;
a group is two A tiles of 32 targets, and a chunk -- the proof's unit -- is one
A tile seen by one lane half: target k lies in chunk
4 (k >> 6) + 2 ((k >> 5) & 1) + ((k >> 2) & 1).  Every case compares the
forward (distances, argmins) and the gradients bit for bit with the CPU oracle,
for variant 20 and for the product library's default entry.  In a launch with
clouds of n and m points, direction 1 screens n queries against m targets and
direction 2 the reverse.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDE = 20
ENTRIES = (WIDE, None)  # the wide variant of the tuning build, the product library's default entry


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


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _assert_equal(out, ref, what, grads=True):
    d1, d2, i1, i2, _, g1, g2 = out
    r1, r2, j1, j2, gr1, gr2 = ref
    np.testing.assert_array_equal(i1.cpu().numpy(), j1, err_msg=what)
    np.testing.assert_array_equal(i2.cpu().numpy(), j2, err_msg=what)
    np.testing.assert_array_equal(_bits(d1.cpu().numpy()), _bits(r1), err_msg=what)
    np.testing.assert_array_equal(_bits(d2.cpu().numpy()), _bits(r2), err_msg=what)
    if grads:
        np.testing.assert_array_equal(_bits(g1.cpu().contiguous().numpy()), _bits(gr1), err_msg=what)
        np.testing.assert_array_equal(_bits(g2.cpu().contiguous().numpy()), _bits(gr2), err_msg=what)


def _check(cuda, oracle, a, c, grads=True):
    """Variant 20 and the default entry on row clouds; returns the last one's argmins of direction 1."""
    import pcm_hip
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    ref, (w1, w2) = _reference(oracle, a, c)
    x1, x2 = a.to(cuda), c.to(cuda)
    for v in ENTRIES:
        out = _outputs(cuda, b, n, m)
        pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, variant=v)
        torch.cuda.synchronize()
        _assert_equal(out, ref, f"variant {v}, n={n}, m={m}", grads)
    return out[2].cpu().numpy()


def _clouds(seed, b, n, m):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g), torch.rand(b, m, 3, generator=g)


@pytest.mark.parametrize("nt", [128, 129, 192, 256, 257, 320, 448, 512, 513, 576, 768, 832, 960, 961])
def test_mfma_wide_group_counts(cuda, oracle, nt):
    # 2..16 target groups: a wave runs 0, 1, 2, 3 or 4 of them, its last group
    # re-reads itself, the cloud's last group is part padding where nt is no
    # multiple of 64, and with 64 (or 257 = 256 + 1) queries a query half holds
    # fewer than 128 live ones; the fold and the two updates that cross from
    # one group into the next run once per further group
    for nq in (64, 257):
        a, c = _clouds(5000 * nt + nq, 2, nq, nt)
        _check(cuda, oracle, a, c)


def test_mfma_wide_winner_in_every_position(cuda, oracle):
    # batch element r: query k sits within 1e-4 of target 4 k + r, so over the
    # four elements every target -- every (group, A tile, lane half, row block
    # j, row r) of the screen -- is the argmin of some query, and every query
    # column of the workgroup has an argmin planted
    b, nq, nt = 4, 256, 1024
    g = torch.Generator().manual_seed(2424)
    c = torch.rand(b, nt, 3, generator=g)
    off = (torch.rand(b, nq, 3, generator=g) * 2.0 - 1.0) * 1e-4
    want = 4 * np.arange(nq)[None, :] + np.arange(b)[:, None]
    a = torch.stack([c[r, want[r]] for r in range(b)]) + off
    i1 = _check(cuda, oracle, a, c)
    np.testing.assert_array_equal(i1, want.astype(np.int32))


def _chunk_of(k):
    return 4 * (k >> 6) + 2 * ((k >> 5) & 1) + ((k >> 2) & 1)


def _chunk_slots(ch):
    """The 16 targets of wide chunk ch, ascending."""
    base = 64 * (ch >> 2) + 32 * ((ch >> 1) & 1) + 4 * (ch & 1)
    return [base + 8 * j + r for j in range(4) for r in range(4)]


def _planted_near_ties(seed):
    """64 queries on a jittered 4 x 4 x 4 grid (coordinates multiples of 2^-10)
    and 1024 random targets, of which each query gets a planted pair far nearer
    than any random one.  Queries 0..31: two targets at exactly the same
    distance (q -+ 2^-9 along one axis, both exact in fp32), the lower index
    must win.  Queries 32..63: offsets (d, 0, 0) and (d, e, 0) rotated over the
    axes with d = 3 * 2^-10, e = 2^-20 -- d^2 and d^2 + e^2 are exact in fp32
    and one ulp apart; the nearer one sits at the higher index.  Query j's first
    target lies in chunk j; the second in (a) the same chunk, (b) another chunk
    of the same quarter, (c) a chunk of another quarter, by j mod 3.  Returns
    the clouds, the planted argmins and each query's kind."""
    rng = np.random.default_rng(seed)
    nq, nt = 64, 1024
    grid = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    q = (grid * 256 + 128 + rng.integers(-32, 33, (nq, 3))) / 1024.0
    t = rng.random((nt, 3))
    used, want, kinds = set(), np.zeros(nq, np.int64), []
    for j in range(nq):
        kind = "abc"[j % 3]
        ch_a = j
        if kind == "a":
            ch_b = ch_a
        elif kind == "b":  # same quarter: the other lane half, the other A tile, or four groups on
            ch_b = (ch_a ^ 1, ch_a ^ 2, (ch_a + 16) % 64)[(j // 3) % 3]
        else:  # another quarter: one or two groups on
            ch_b = (ch_a + (4, 8)[(j // 3) % 2]) % 64
        assert (((ch_a >> 2) & 3) == ((ch_b >> 2) & 3)) == (kind != "c")

        def free_slot(ch, start):
            slots = _chunk_slots(ch)
            for s in range(16):
                k = slots[(start + s) % 16]
                if k not in used:
                    used.add(k)
                    return k
            raise AssertionError("chunk full")
        ka = free_slot(ch_a, 5 * j)
        # (a): the second target in the other part's half of the chunk (row blocks j ^ 2)
        kb = free_slot(ch_b, 5 * j + (8 if kind == "a" else 3))
        assert ka != kb and _chunk_of(ka) == ch_a and _chunk_of(kb) == ch_b
        axis, ax2 = j % 3, (j + 1) % 3
        lo, hi = min(ka, kb), max(ka, kb)
        if j < 32:
            d = 2.0 ** -9
            t[lo] = q[j]
            t[lo, axis] += d
            t[hi] = q[j]
            t[hi, axis] -= d
            want[j] = lo
        else:
            d, e = 3 * 2.0 ** -10, 2.0 ** -20
            t[hi] = q[j]
            t[hi, axis] += d
            t[lo] = q[j]
            t[lo, axis] += d
            t[lo, ax2] += e
            want[j] = hi
        kinds.append(kind)
    q32, t32 = q.astype(np.float32), t.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q)  # the planted coordinates are exact in fp32
    planted = sorted(used)
    assert np.array_equal(t32[planted].astype(np.float64), t[planted])
    return q32, t32, want, kinds


def test_mfma_wide_planted_near_ties(cuda, oracle):
    # the chunk id -> candidate maps of the exact rescan (pair in one chunk:
    # proven, both parts), of the whole-quarter plan (pair in two chunks of one
    # quarter) and of the near-tie pass's single-chunk step (pair in chunks of
    # two quarters)
    b = 2
    qs, ts, wants = [], [], []
    for e in range(b):
        q, t, want, kinds = _planted_near_ties(600 + e)
        d = ((q[:, None, :].astype(np.float64) - t[None, :, :]) ** 2).sum(-1)
        srt = np.sort(d, axis=1)
        # float64: the pair is tied or 1 fp32 ulp apart, every other target far outside the screen's bound
        assert np.all(srt[:, 1] - srt[:, 0] <= srt[:, 0] * 2.0 ** -22) and np.all(srt[:, 2] > 4.0 * srt[:, 1])
        assert {k: kinds.count(k) for k in "abc"} == {"a": 22, "b": 21, "c": 21}
        qs.append(q)
        ts.append(t)
        wants.append(want)
    a, c = torch.from_numpy(np.stack(qs)), torch.from_numpy(np.stack(ts))
    i1 = _check(cuda, oracle, a, c)
    np.testing.assert_array_equal(i1, np.stack(wants).astype(np.int32))


@pytest.mark.parametrize("kind", ["milli", "kilo", "offset", "nonfinite"])
def test_mfma_wide_scale_and_offset(cuda, oracle, kind):
    a, c = _clouds(88, 2, 320, 320)
    if kind == "milli":
        a, c = a * 1e-3, c * 1e-3
    elif kind == "kilo":
        a, c = a * 1e3, c * 1e3
    elif kind == "offset":
        a, c = a + 100.0, c + 100.0
    else:  # one non-finite coordinate: its workgroups take the reference scan
        c[1, 7, 2] = float("inf")
    # (the oracle's backward of a non-finite cloud is not the contract: forward only)
    _check(cuda, oracle, a, c, grads=kind != "nonfinite")


@pytest.mark.parametrize("lays", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_mfma_wide_layout_instances(cuda, oracle, lays):
    # the default entry's four layout instances (rows or channel planes per
    # cloud), each its own instantiation of the loop, at an odd size
    import pcm_hip
    b, n, m = 2, 257, 193
    a, c = _clouds(78, b, n, m)
    ref, (w1, w2) = _reference(oracle, a, c)
    x1 = a.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[0] else a.to(cuda)
    x2 = c.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[1] else c.to(cuda)
    assert (pcm_hip.cloud_layout(x1), pcm_hip.cloud_layout(x2)) == lays
    out = _outputs(cuda, b, n, m, planes1=bool(lays[0]), planes2=bool(lays[1]))
    pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, layouts=lays)
    torch.cuda.synchronize()
    _assert_equal(out, ref, f"layouts {lays}")
