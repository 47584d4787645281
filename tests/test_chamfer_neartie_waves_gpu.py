"""Near ties of the one-launch Chamfer step's matrix-core forward, resolved
inside the waves that hold the query (csrc/chamfer_filt.hip filt_forward_mfma:
fused variants 20, 19 and 6 of the tuning build and the product library's
default entry).

Query j of a 256-query workgroup is thread slot j: lane j mod 64 of waves
j / 64 (part 0) and j / 64 + 4 (part 1).  A query whose best chunk is not
proven against the rest is "listed": its wave walks the listed lanes, the
j-th one falling to part j mod 2, and scans the query's plan exactly -- a whole
quarter (the 64-target groups q, q + 4, ..) where that quarter's second-best
chunk may hold the answer, a quarter's best chunk alone where only that one
may.  A chunk is 16 targets: target k lies in chunk
4 (k >> 6) + 2 ((k >> 5) & 1) + ((k >> 2) & 1) of the wide form (variant 20,
the default) and in chunk 4 (k >> 6) + ((k >> 2) & 3) of the narrow one (19,
6); its quarter is (k >> 6) & 3 in both.

Every case compares distances, argmins and both gradients bit for bit with the
CPU oracle, and first asserts in float64, on the CPU, that it produces the
situation it names (_situation below): a planted query's two nearest targets
are tied or one fp32 ulp apart and lie in different chunks under both maps --
so no forward can prove its best chunk and the loop must take it -- while
every other query's best chunk leads by far more than the proof asks for.
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ENTRIES = (20, 19, 6, None)  # wide, narrow, narrow with the earlier hand-off; the product library's default entry
QW = 256                     # queries per workgroup
U80 = 80.0 * 2.0 ** -24      # the proof's bound: E = 80 u r^2 (kFiltU80)


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


def _assert_equal(out, ref, what):
    d1, d2, i1, i2, _, g1, g2 = out
    r1, r2, j1, j2, gr1, gr2 = ref
    np.testing.assert_array_equal(i1.cpu().numpy(), j1, err_msg=what)
    np.testing.assert_array_equal(i2.cpu().numpy(), j2, err_msg=what)
    np.testing.assert_array_equal(_bits(d1.cpu().numpy()), _bits(r1), err_msg=what)
    np.testing.assert_array_equal(_bits(d2.cpu().numpy()), _bits(r2), err_msg=what)
    np.testing.assert_array_equal(_bits(g1.cpu().contiguous().numpy()), _bits(gr1), err_msg=what)
    np.testing.assert_array_equal(_bits(g2.cpu().contiguous().numpy()), _bits(gr2), err_msg=what)


def _check(cuda, oracle, a, c):
    """Every entry on row clouds [b, n, 3], [b, m, 3] (numpy or torch); returns the oracle's argmins of direction 1."""
    import pcm_hip
    a, c = torch.as_tensor(a), torch.as_tensor(c)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    assert b <= 4
    ref, (w1, w2) = _reference(oracle, a, c)
    x1, x2 = a.to(cuda), c.to(cuda)
    for v in ENTRIES:
        out = _outputs(cuda, b, n, m)
        pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, variant=v)
        torch.cuda.synchronize()
        _assert_equal(out, ref, f"variant {v}, n={n}, m={m}")
    return ref[2]


def _chunks(nt):
    """Chunk of every target under the wide and the narrow map."""
    k = np.arange(nt)
    return 4 * (k >> 6) + 2 * ((k >> 5) & 1) + ((k >> 2) & 1), 4 * (k >> 6) + ((k >> 2) & 3)


def _situation(q, t):
    """Float64 restatement of the proof's two sure verdicts for every query
    of direction 1 (queries q [nq, 3] against targets t [nt, 3], fp32 values).

    With d the exact squared distances, gap = (least d outside the chunk of
    the lexicographic argmin) - (least d), the larger of the two chunk maps'
    for `proven`, the smaller for `listed`.  A screened value is the exact one
    within E_true <= E, where the forward uses E = 80 u min((R + |q'|)^2,
    (2 |q'| + sqrt(d_b))^2) with q', R about the workgroup's query centre and
    d_b >= the least d; the best chunk is proven when second - best > 2 E.
      listed: gap = 0, or gap <= E_low / 10 with E_low a lower bound of E --
              second - best <= gap + 2 E_true, and the error analysis leaves
              E_true <= (59 / 80) E, so this stays below 2 E: never proven;
      proven: gap > 4 E_up with E_up = 80 u (R + |q'|)^2, an upper bound of
              E: second - best >= gap - 2 E_true > 2 E.
    Returns (listed, proven, argmin), the margins 1 % wide for the forward's
    own fp32 rounding."""
    q, t = q.astype(np.float64), t.astype(np.float64)
    nq, nt = len(q), len(t)
    d = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    best = d.min(1)
    arg = d.argmin(1)  # the first of equals: the lowest index
    listed, proven = np.ones(nq, bool), np.ones(nq, bool)
    for w0 in range(0, nq, QW):
        sl = slice(w0, min(w0 + QW, nq))
        c = q[sl].mean(0)
        qn = np.linalg.norm(q[sl] - c, axis=1)
        r = np.linalg.norm(t - c, axis=1).max()
        e_up = 1.01 * U80 * (r + qn) ** 2 + 2.0 ** -99
        e_low = 0.99 * U80 * np.minimum((r + qn) ** 2, (2 * qn + np.sqrt(best[sl])) ** 2)
        for ch in _chunks(nt):
            other = np.where(ch[None, :] != ch[arg[sl]][:, None], d[sl], np.inf).min(1)
            gap = other - best[sl]
            listed[sl] &= (gap == 0) | (gap <= 0.1 * e_low)
            proven[sl] &= gap > 4 * e_up
    return listed, proven, arg


# ---- planted clouds ---------------------------------------------------------
# Targets: the sites of a 16 x 8 x 8 lattice of pitch 1/16, jittered by up to
# 2^-7, in a seeded random index order -- any two at least 0.046 apart.  A
# query sits within 2^-10 per axis of its home target, so its best chunk leads
# by 2e-3 where the proof asks for < 3e-5.  A planted query j has its pair
# (lo < hi) moved to q -+ 2^-9 along one axis (an exact tie: lo must win) or to
# q + (d, e, 0) for lo and q + (d, 0, 0) for hi with d = 3 * 2^-10, e = 2^-20
# (d^2 and d^2 + e^2 are exact in fp32 and one ulp apart: hi must win).  All
# coordinates are multiples of 2^-20 below 1, exact in fp32.
def _planted(seed, nq, nt, plants):
    """plants: {query: (lo, hi)}.  Returns q [nq, 3], t [nt, 3] (fp32) and {query: wanted argmin}."""
    rng = np.random.default_rng(seed)
    sites = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    sites = sites[rng.permutation(1024)][:nt]
    t = (sites * 256 + 128 + rng.integers(-32, 33, (nt, 3))) / 4096.0
    moved = {k for pair in plants.values() for k in pair}
    assert len(moved) == 2 * len(plants) and max(moved, default=0) < nt
    free = np.array([k for k in range(nt) if k not in moved])
    home = free[rng.integers(0, len(free), nq)]
    for j, (lo, _) in plants.items():
        home[j] = lo
    q = t[home] + rng.integers(-16, 17, (nq, 3)) / 16384.0
    want = {}
    for n_, (j, (lo, hi)) in enumerate(sorted(plants.items())):
        assert lo < hi
        axis, ax2 = n_ % 3, (n_ + 1) % 3
        if n_ % 2 == 0:
            t[lo] = q[j]
            t[lo, axis] += 2.0 ** -9
            t[hi] = q[j]
            t[hi, axis] -= 2.0 ** -9
            want[j] = lo
        else:
            t[hi] = q[j]
            t[hi, axis] += 3 * 2.0 ** -10
            t[lo] = t[hi]
            t[lo, ax2] += 2.0 ** -20
            want[j] = hi
    q32, t32 = q.astype(np.float32), t.astype(np.float32)
    assert np.array_equal(q32.astype(np.float64), q) and np.array_equal(t32.astype(np.float64), t)
    return q32, t32, want


def _assert_planted(q, t, want):
    """Exactly the planted queries are listed, every other one is proven, and the planted argmins win."""
    listed, proven, arg = _situation(q, t)
    assert sorted(np.flatnonzero(listed)) == sorted(want), "the listed queries are the planted ones"
    assert np.all(listed ^ proven), "every query is surely listed or surely proven"
    for j, k in want.items():
        assert arg[j] == k
    d = np.sort(((q[sorted(want), None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1), axis=1)
    # the pair is tied or one fp32 ulp apart, every other target far outside the bound
    assert np.all(d[:, 1] - d[:, 0] <= d[:, 0] * 2.0 ** -22) and np.all(d[:, 2] > 100.0 * d[:, 1])


def _run_planted(cuda, oracle, cases):
    """cases: (seed, nq, nt, plants) of one shape, up to four -- one launch per entry."""
    qs, ts, wants = [], [], []
    for seed, nq, nt, plants in cases:
        q, t, want = _planted(seed, nq, nt, plants)
        _assert_planted(q, t, want)
        qs.append(q)
        ts.append(t)
        wants.append(want)
    i1 = _check(cuda, oracle, np.stack(qs), np.stack(ts))
    for e, want in enumerate(wants):
        for j, k in want.items():
            assert i1[e, j] == k


# pairs in different chunks under both maps: the same quarter (four groups
# on: a whole-quarter plan) or quarters 0/1 against 2/3 (two groups on: the
# single-chunk step of two quarters)
def _pair(k, arrangement):
    return (k, k + 256) if arrangement == "quarter" else (k, k + 128)


@pytest.mark.parametrize("arrangement", ["quarter", "across"])
@pytest.mark.parametrize("wave", [0, 1, 2, 3])
def test_one_near_tie_in_every_lane_position(cuda, oracle, wave, arrangement):
    # one listed query per batch element, in lane 0, 31, 32, 63 of the wave;
    # exact ties (the lower index wins) and one-ulp pairs (the higher one
    # does) alternate over the cases, the pair's first target moves over the
    # groups 0..3 (quarter) or 0, 1 (across)
    cases = []
    for e, lane in enumerate((0, 31, 32, 63)):
        k = 64 * ((wave + e) % (4 if arrangement == "quarter" else 2)) + 7 * lane % 64
        plants = {64 * wave + lane: _pair(k, arrangement)}
        cases.append((1000 + 16 * wave + e, 256, 1024, plants))
    _run_planted(cuda, oracle, cases)


@pytest.mark.parametrize("lanes", [(10, 11), (0, 1, 63), (5, 6, 7, 31, 32)])
def test_several_near_ties_in_one_wave(cuda, oracle, lanes):
    # 2, 3 and 5 listed queries in one wave and none elsewhere: both parts'
    # waves run the loop, the listed lanes alternating between them; batch
    # element e plants them in wave e
    cases = []
    for wave in range(4):
        plants = {64 * wave + lane: _pair(64 * (i % 2) + 3 * lane % 64 + 512 * (i // 2 % 2), ("quarter", "across")[i % 2])
                  for i, lane in enumerate(lanes)}
        cases.append((2000 + 10 * len(lanes) + wave, 256, 1024, plants))
    _run_planted(cuda, oracle, cases)


def test_a_whole_wave_listed(cuda, oracle):
    # all 64 lanes of one wave (element e: wave e) and none elsewhere: each
    # part's wave runs 32 iterations
    cases = []
    for wave in range(4):
        plants = {64 * wave + lane: _pair(lane + 512 * (lane & 1), ("quarter", "across")[(lane >> 1) & 1])
                  for lane in range(64)}
        cases.append((3000 + wave, 256, 1024, plants))
    _run_planted(cuda, oracle, cases)


def test_a_whole_workgroup_listed_duplicated_targets(cuda, oracle):
    # every target again at index k + 512: each query's nearest is an exact tie
    # of two chunks, so every query is listed and each argmin is below 512
    g = torch.Generator().manual_seed(31)
    a = torch.rand(2, 256, 3, generator=g)
    c = torch.rand(2, 512, 3, generator=g)
    c = torch.cat([c, c], dim=1)
    for e in range(2):
        listed, _, arg = _situation(a[e].numpy(), c[e].numpy())
        assert listed.all() and arg.max() < 512
    i1 = _check(cuda, oracle, a, c)
    assert i1.max() < 512


def test_a_whole_workgroup_listed_collapsed_targets(cuda, oracle):
    # every target the same point: every chunk ties with every other, each
    # query is listed with four whole quarters, every argmin is 0
    g = torch.Generator().manual_seed(32)
    a = torch.rand(2, 256, 3, generator=g)
    c = torch.rand(2, 1, 3, generator=g).expand(2, 1024, 3).contiguous()
    for e in range(2):
        listed, _, arg = _situation(a[e].numpy(), c[e].numpy())
        assert listed.all() and not arg.any()
    i1 = _check(cuda, oracle, a, c)
    assert not i1.any()


def test_integer_lattice(cuda, oracle):
    # targets: the 1000 points of a 10^3 integer lattice in random order;
    # queries: cell centres, each exactly 0.75 from its cell's eight corners
    rng = np.random.default_rng(33)
    cells = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), -1).reshape(-1, 3)
    t = np.stack([cells[rng.permutation(1000)] for _ in range(2)]).astype(np.float32)
    q = (rng.integers(0, 9, (2, 256, 3)) + 0.5).astype(np.float32)
    for e in range(2):
        listed, _, _ = _situation(q[e], t[e])
        d = ((q[e][:, None, :].astype(np.float64) - t[e][None].astype(np.float64)) ** 2).sum(-1)
        assert np.all((d == 0.75).sum(1) == 8) and d.min() == 0.75
        assert listed.sum() >= 250  # (a query's eight corners in one chunk: as good as never)
    _check(cuda, oracle, q, t)


@pytest.mark.parametrize("nt", [129, 961, 1000])
@pytest.mark.parametrize("nq", [64, 257])
def test_ragged_sizes(cuda, oracle, nq, nt):
    # nt = 129: three groups, so a quarter is one group at most, and the last
    # group holds one live target; 961: the sixteenth group holds one; 1000: it
    # holds 40.  Pairs: inside one group (k, k ^ 4: a whole quarter of fewer
    # than four groups at nt = 129), from another quarter into the last live
    # target (the part-padding group's single chunk, clamped), in the
    # part-padding group's own quarter (a whole quarter whose last group is
    # part padding) and inside that group where it holds enough.  nq = 257: the
    # second workgroup's one live query, lane 0 of wave 0, is planted too.
    def inside(k):
        return min(k, k ^ 4), max(k, k ^ 4)
    last = nt - 1
    grp = last >> 6
    own = 64 * (grp % 4)  # the first group of the last group's quarter
    pairs = [inside(9),
             (64 * ((grp + 2) % 4) + 21, last),
             (own + 33, own + 33 + 256) if grp >= 8 else inside(104),
             (64 * grp + 2, 64 * grp + 6) if last - 64 * grp >= 7 else inside(70)]
    lanes = [0, 13, 14, 63]
    plants = {lane: pair for lane, pair in zip(lanes, pairs)}
    if nq == 257:
        plants[256] = inside(64 + 50)
    cases = [(4000 + nt + nq + e, nq, nt, plants) for e in range(2)]
    _run_planted(cuda, oracle, cases)


def test_large_bound_two_clusters(cuda, oracle):
    # two tight clusters 100 apart: the query centre lies between them, R and
    # |q'| are ~87, E ~ 0.14 against cluster diameters of 0.17 -- most queries
    # cannot be proven and scan whole quarters
    g = torch.Generator().manual_seed(34)
    a = torch.rand(2, 320, 3, generator=g) * 0.1
    c = torch.rand(2, 448, 3, generator=g) * 0.1
    a[:, 1::2] += 100.0
    c[:, ::3] += 100.0
    for e in range(2):
        listed, proven, _ = _situation(a[e].numpy(), c[e].numpy())
        assert listed.mean() > 0.5 and not proven.any()
    _check(cuda, oracle, a, c)


@pytest.mark.parametrize("lays", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_planted_near_ties_in_every_layout_instance(cuda, oracle, lays):
    # the default entry's four layout instances (rows or channel planes per
    # cloud), each its own instantiation of the loop
    import pcm_hip
    plants = {3: _pair(40, "quarter"), 4: _pair(100, "across"), 130: _pair(77, "across"), 255: _pair(201, "quarter")}
    q, t, want = _planted(5000, 256, 1000, plants)
    _assert_planted(q, t, want)
    a, c = torch.from_numpy(np.stack([q, q])), torch.from_numpy(np.stack([t, t]))
    b, n, m = 2, 256, 1000
    ref, (w1, w2) = _reference(oracle, a, c)
    x1 = a.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[0] else a.to(cuda)
    x2 = c.transpose(1, 2).contiguous().to(cuda).transpose(1, 2) if lays[1] else c.to(cuda)
    assert (pcm_hip.cloud_layout(x1), pcm_hip.cloud_layout(x2)) == lays
    out = _outputs(cuda, b, n, m, planes1=bool(lays[0]), planes2=bool(lays[1]))
    pcm_hip.chamfer_loss_grad(x1, x2, w1, w2, *out, layouts=lays)
    torch.cuda.synchronize()
    _assert_equal(out, ref, f"layouts {lays}")
    for j, k in want.items():
        assert ref[2][0, j] == k


def test_the_benchmarks_own_clouds(cuda, oracle):
    # bench.py's seeded clouds (rank 0), first two elements, n = m = 1024
    sys.path.insert(0, REPO)
    import bench
    g = torch.Generator(device="cpu").manual_seed(bench.BENCH_SEED)
    a = torch.rand(bench.B, bench.N, 3, generator=g)[:2].contiguous()
    c = torch.rand(bench.B, bench.M, 3, generator=g)[:2].contiguous()
    assert a.shape == (2, 1024, 3) and c.shape == (2, 1024, 3)
    # (uniform clouds: a handful of queries can be neither proven nor surely listed; one surely is)
    assert sum(_situation(a[e].numpy(), c[e].numpy())[0].sum() for e in range(2)) >= 1
    _check(cuda, oracle, a, c)
