"""Ball-query and uniform-loss checks that need no GPU: the library exports and
validates pcm_ball_query / pcm_uniform_loss, the Python layers import without a
device and raise the documented errors, and the numpy restatement of
tests/uniform_restated.py agrees with a float32 torch composition of the op
sequence the loss replaces and with torch autograd, within derived bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import knn_restated as K
import uniform_restated as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3d-pointcloudreconstruction_amd", "csrc")
HEADER = os.path.join(REPO, "include", "pcm.h")

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4
NAN, INF = float("nan"), float("inf")

CASES = [(65, [0.04, 0.08, 0.2]), (130, [0.04, 0.08, 0.2]), (300, [0.04, 0.08, 0.2]),
         (1024, [0.004, 0.006, 0.008, 0.010, 0.012])]


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _floats(values):
    return (ctypes.c_float * len(values))(*values)


def _doubles(values):
    return (ctypes.c_double * len(values))(*values)


def test_library_exports_and_constants_agree():
    import pcm_hip
    lib = pcm_hip.load_library()
    src = open(HEADER).read()
    for name in ("pcm_ball_query", "pcm_uniform_loss", "pcm_uniform_workspace_bytes"):
        assert name in pcm_hip.EXPORTED
        assert hasattr(lib, name)
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
    assert pcm_hip.BALL_MAX_NSAMPLE == int(re.search(r"#define\s+PCM_BALL_MAX_NSAMPLE\s+(\d+)", src).group(1)) == 64
    assert pcm_hip.UNIFORM_MAX_SCALES == int(re.search(r"#define\s+PCM_UNIFORM_MAX_SCALES\s+(\d+)", src).group(1)) == 8
    hip = open(os.path.join(CSRC, "grouping.hip")).read()
    assert pcm_hip.BALL_TILE == int(re.search(r"kBallTile\s*=\s*(\d+)", hip).group(1))
    assert pcm_hip.BALL_CENTRES == int(re.search(r"kBallWaves\s*=\s*(\d+)", hip).group(1))
    import loss
    assert loss.UNIFORM_MAX_NSAMPLE == pcm_hip.BALL_MAX_NSAMPLE
    # the padding rule is documented as unverified wherever it is stated
    assert "NOT verified" in src and "NOT verified" in hip
    # the source keeps to the other kernels' conventions: pcm_wg_or and DPP steps, no generic
    # workgroup votes, no __shfl chains, no atomics, no waiting between workgroups
    lines = [ln.split("//", 1)[0] for ln in hip.splitlines()]
    assert not [ln for ln in lines if "__syncthreads_or" in ln or "__syncthreads_and" in ln or
                "__syncthreads_count" in ln]
    assert not [ln for ln in lines if "__shfl" in ln]
    assert not [ln for ln in lines if "atomic" in ln.lower() or "s_sleep" in ln]
    assert "pcm_wg_or" in hip and "pcm_wave_sum_f64" in hip


def test_workspace_size():
    import pcm_hip
    lib = pcm_hip.load_library()

    def need(b, n, npoint, ns):
        return lib.pcm_uniform_workspace_bytes(b, n, npoint, len(ns), _ints(ns))

    # per seed its index, a double and its coordinates, then 8 + 12 bytes per slot record
    assert need(2, 300, 15, [12, 24, 60]) == 2 * 15 * 28 + 2 * 15 * 96 * 20
    assert need(0, 300, 15, [12, 24]) == 0 and need(-1, 300, 15, [12]) == 0
    assert need(2, 0, 15, [12]) == 0 and need(2, 300, 0, [12]) == 0
    assert need(2, 300, 15, [1]) == 0 and need(2, 300, 15, []) == 0 and need(2, 300, 15, [2] * 9) == 0
    assert lib.pcm_uniform_workspace_bytes(2, 300, 15, 1, None) == 0
    # monotone in every size
    base = need(2, 300, 15, [12, 24])
    assert need(3, 300, 15, [12, 24]) > base and need(2, 300, 16, [12, 24]) > base
    assert need(2, 300, 15, [12, 25]) > base and need(2, 300, 15, [12, 24, 2]) > base
    assert need(2, 301, 15, [12, 24]) >= base


def _host_pointer():
    # a non-null, 8-byte aligned pointer to host memory, never dereferenced: every call below is rejected first
    buf = ctypes.create_string_buffer(4096 + 8)
    addr = (ctypes.addressof(buf) + 7) & ~7
    return buf, ctypes.c_void_p(addr)


def test_ball_query_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None

    def call(b=2, n=8, s=3, lx=0, lc=0, radius=0.5, nsample=4, xyz=one, new=one, idx=one, cnt=one):
        return lib.pcm_ball_query(xyz, new, b, n, s, lx, lc, radius, nsample, idx, cnt, null)

    assert call(b=-1) == INVALID and call(n=-8) == INVALID and call(s=-1) == INVALID
    assert call(lx=2) == INVALID and call(lc=-1) == INVALID
    assert call(nsample=0) == INVALID and call(nsample=-2) == INVALID
    for r in (0.0, -0.5, NAN, INF, -INF):
        assert call(radius=r) == INVALID
    assert call(b=0, nsample=0) == INVALID and call(b=0, radius=0.0) == INVALID  # before the b == 0 rule
    # then b == 0 is a no-op, also with null pointers
    assert call(b=0, xyz=null, new=null, idx=null, cnt=null) == OK
    assert call(b=0, n=0, s=0, xyz=null, new=null, idx=null, cnt=null) == OK
    assert call(n=0) == INVALID and call(s=0) == INVALID
    assert call(xyz=null) == INVALID and call(new=null) == INVALID and call(idx=null) == INVALID
    assert call(nsample=pcm_hip.BALL_MAX_NSAMPLE + 1) == UNSUPPORTED
    assert call(n=pcm_hip.KNN_MAX_POINTS + 1) == UNSUPPORTED
    assert call(n=0, nsample=pcm_hip.BALL_MAX_NSAMPLE + 1) == INVALID  # invalid comes first
    del keep


def test_uniform_loss_rejects_bad_arguments_without_device():
    import pcm_hip
    lib = pcm_hip.load_library()
    keep, one = _host_pointer()
    null = None
    big = 1 << 30
    good_ns, good_r, good_w = [4, 6], [0.1, 0.2], [0.5, 0.25]

    def call(b=2, n=80, layout=0, npoint=4, nscales=2, ns=good_ns, radii=good_r, w=good_w, L=0.2, xyz=one,
             loss=one, grad=null, groups=null, ws=one, ws_bytes=big):
        return lib.pcm_uniform_loss(xyz, b, n, layout, npoint, nscales, None if ns is None else _ints(ns),
                                    None if radii is None else _floats(radii), None if w is None else _doubles(w),
                                    L, loss, grad, groups, ws, ws_bytes, null)

    assert call(b=-1) == INVALID and call(n=-8) == INVALID and call(layout=2) == INVALID
    assert call(nscales=0) == INVALID and call(nscales=pcm_hip.UNIFORM_MAX_SCALES + 1) == INVALID
    assert call(ns=None) == INVALID and call(radii=None) == INVALID and call(w=None) == INVALID
    assert call(npoint=0) == INVALID and call(npoint=-3) == INVALID
    assert call(ns=[4, 1]) == INVALID and call(ns=[0, 6]) == INVALID
    for bad in (NAN, INF, 0.0, -0.1):
        assert call(radii=[0.1, bad]) == INVALID
        assert call(L=bad) == INVALID
    for bad in (NAN, INF, -INF):
        assert call(w=[bad, 0.25]) == INVALID
    assert call(w=[-1.0, 0.0], ws=null) == WORKSPACE  # a weight only has to be finite
    assert call(b=0, ns=[4, 1]) == INVALID  # before the b == 0 rule
    # then b == 0 is a no-op and writes nothing
    assert call(b=0, xyz=null, loss=null, ws=null, ws_bytes=0) == OK
    assert call(n=0) == INVALID and call(xyz=null) == INVALID and call(loss=null) == INVALID
    assert call(ns=[4, pcm_hip.BALL_MAX_NSAMPLE + 1]) == UNSUPPORTED
    assert call(ns=[pcm_hip.BALL_MAX_NSAMPLE, 2], ws=null) == WORKSPACE  # 64 is supported
    assert call(n=pcm_hip.KNN_MAX_POINTS + 1) == UNSUPPORTED
    assert call(ws=null) == WORKSPACE
    assert call(ws_bytes=lib.pcm_uniform_workspace_bytes(2, 80, 4, 2, _ints(good_ns)) - 1) == WORKSPACE
    assert call(ws=ctypes.c_void_p(one.value + 4)) == INVALID  # not 8-byte aligned
    del keep


def test_modules_import_without_a_device_and_raise_on_bad_input():
    import loss
    import pointnet2_utils as pn2
    import uniform_loss
    for doc in (pn2.__doc__, uniform_loss.__doc__, loss.Loss.get_uniform_loss.__doc__):
        assert "not verified" in " ".join(doc.split()) or "unverified" in doc
    assert "PU-GAN's own formula differs" in " ".join(loss.Loss.get_uniform_loss.__doc__.split())
    cloud = torch.rand(2, 100, 3)
    centres = cloud[:, :4]
    # no CPU path
    with pytest.raises(RuntimeError):
        pn2.ball_query(0.2, 4, cloud, centres)
    with pytest.raises(RuntimeError):
        pn2.ball_query_count(0.2, 4, cloud, centres)
    with pytest.raises(RuntimeError):
        pn2.furthest_point_sample(cloud, 4)
    with pytest.raises(TypeError):
        pn2.ball_query(0.2, 4, cloud.double(), centres.double())
    with pytest.raises(ValueError):
        pn2.ball_query(0.2, 4, cloud[:, :, :2], centres)
    with pytest.raises(ValueError):
        pn2.ball_query(0.2, 0, cloud, centres)
    with pytest.raises(ValueError):
        pn2.furthest_point_sample(cloud, 0)
    # the gathers are torch indexing: any device, differentiable in the features
    feats = torch.rand(2, 5, 100, dtype=torch.float64, requires_grad=True)
    idx2 = torch.randint(0, 100, (2, 7), dtype=torch.int32)
    idx3 = torch.randint(0, 100, (2, 7, 3), dtype=torch.int32)
    got2, got3 = pn2.gather_operation(feats, idx2), pn2.grouping_operation(feats, idx3)
    assert got2.shape == (2, 5, 7) and got3.shape == (2, 5, 7, 3)
    for bi in range(2):
        assert torch.equal(got2[bi], feats[bi][:, idx2[bi].long()])
        assert torch.equal(got3[bi], feats[bi][:, idx3[bi].long()])
    (got2.sum() + 2 * got3.sum()).backward()
    want = np.zeros((2, 100))
    for bi in range(2):
        np.add.at(want[bi], idx2[bi].numpy(), 1)
        np.add.at(want[bi], idx3[bi].numpy().ravel(), 2)
    assert np.array_equal(feats.grad.numpy(), np.broadcast_to(want[:, None, :], (2, 5, 100)))

    L = loss.Loss()
    with pytest.raises(RuntimeError):
        L.get_uniform_loss(cloud, percentage=[0.04, 0.08])
    with pytest.raises(TypeError):
        L.get_uniform_loss(cloud.double(), percentage=[0.04, 0.08])
    with pytest.raises(ValueError, match="0.05"):
        L.get_uniform_loss(torch.rand(2, 19, 3))  # no seed
    with pytest.raises(ValueError, match="0.004"):
        L.get_uniform_loss(cloud)  # int(100 * 0.004) = 0 points a group
    with pytest.raises(ValueError, match="0.019"):
        L.get_uniform_loss(cloud, percentage=[0.04, 0.019])  # one point
    with pytest.raises(ValueError, match="0.65"):
        L.get_uniform_loss(cloud, percentage=[0.04, 0.65])  # 65 points
    with pytest.raises(ValueError):
        L.get_uniform_loss(cloud, percentage=[])
    with pytest.raises(ValueError):
        L.get_uniform_loss(cloud[:, :, :2], percentage=[0.04])
    fn = uniform_loss.uniform_lossFunction.apply
    with pytest.raises(ValueError):
        fn(cloud, 5, [1], [0.2], [1.0], 0.2)
    with pytest.raises(ValueError):
        fn(cloud, 5, [65], [0.2], [1.0], 0.2)
    with pytest.raises(ValueError):
        fn(cloud, 0, [4], [0.2], [1.0], 0.2)
    with pytest.raises(ValueError):
        fn(cloud, 5, [4] * 9, [0.2] * 9, [1.0] * 9, 0.2)


def test_restated_rules_on_small_inputs():
    cloud = np.array([[[0, 0, 0], [0.5, 0, 0], [0.25, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0.1, 0, 0],
                       [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0]]], np.float32)
    centres = np.array([[[0, 0, 0], [9, 9, 9], [np.nan, 0, 0]]], np.float32)
    idx, cnt, hits = U.ball_query_restated(cloud, centres, 0.5, 3)
    # exactly r2 is outside, its neighbour towards the centre inside; NaN and inf points are never hits;
    # the first three hits in index order, not the nearest
    assert idx[0, 0].tolist() == [0, 2, 5] and cnt[0, 0] == 3 and hits[0, 0] == 4
    assert idx[0, 1].tolist() == [0, 0, 0] and cnt[0, 1] == 0
    assert idx[0, 2].tolist() == [0, 0, 0] and cnt[0, 2] == 0
    idx, cnt, _ = U.ball_query_restated(cloud, centres, 0.5, 6)
    assert idx[0, 0].tolist() == [0, 2, 5, 6, 0, 0] and cnt[0, 0] == 4  # the first hit pads
    idx, cnt, _ = U.ball_query_restated(cloud[:, 1:], centres, 0.3, 4)
    assert idx[0, 0].tolist() == [1, 4, 1, 1] and cnt[0, 0] == 2  # the first hit, not index 0
    # the seeds follow pcm_fps
    seeds = U.fps_restated(np.array([[[0, 0, 0], [1, 0, 0], [0.4, 0, 0], [1, 0, 0]]], np.float32), 4)
    assert seeds[0].tolist() == [0, 1, 2, 0]


# The op sequence the fused call replaces, composed in float32 torch from the
# project's own description of it: sample, gather the seeds,
# and per percentage query, group, search every group against itself with k = 2,
# take the second column, add 1e-8, average per group, compare with expect_len.
# The sampling, ball query and k-NN are the numpy restatements (there is no
# device here); every float32 operation after them is torch's.
def _composed_f32(xyz, percentage, radius=1.0):
    pts = torch.from_numpy(xyz)
    b, n, _ = pts.shape
    npoint, nsample, ball_radius, _, _ = U.uniform_params(n, percentage, radius)
    seeds = U.fps_restated(xyz, npoint, 0)
    centres = U.gather_points(xyz, seeds)
    expect_len = float(np.sqrt(np.pi * radius ** 2 / n))
    total = 0
    for p, ns, r in zip(percentage, nsample, ball_radius):
        idx, _, _ = U.ball_query_restated(xyz, centres, r, ns)
        grouped = U.gather_points(xyz, idx).reshape(b * npoint, ns, 3)
        d2, _ = K.knn_restated(grouped, grouped, 2)
        dist = torch.sqrt(torch.from_numpy(d2))
        u = torch.abs(dist[:, :, 1:] + 1e-8)
        m = torch.mean(u, dim=1)
        term = (m - expect_len) ** 2 / (expect_len + 1e-8)
        total = total + torch.mean(term) * (p * 100) ** 2
    return float(total / len(percentage))


@pytest.mark.parametrize("kind", ["cube", "shell"])
@pytest.mark.parametrize("n,percentage", CASES)
def test_restatement_agrees_with_the_composed_float32_sequence(kind, n, percentage):
    xyz = U.make_cloud(kind, 3, n, 100 + n)
    npoint, nsample, ball_radius, weight, L = U.uniform_params(n, percentage)
    res = U.uniform_restated(xyz, npoint, nsample, ball_radius, weight, L)
    got = _composed_f32(xyz, percentage)
    # The bound, from the float64 values.  eps = 2^-24.  Per group of ns slots the float32 mean of the
    # same u values is off by at most (ns + 2) eps m (ns - 1 additions, the division, two to spare); L
    # enters rounded to float32 (eps L); both pass through d term / d m = 2 |m - L| / (L + 1e-8) and
    # their square through 1 / (L + 1e-8); the subtraction (twice, squared), the square, the division
    # and the rounded denominator cost 5 eps term.  The mean over the G groups, the product with
    # (100 p)^2, the running sum over the scales and the last division cost at most
    # (G + len(percentage) + 3) eps of the scale's value.
    eps = 2.0 ** -24
    groups = 3 * npoint
    bound = 0.0
    for q, ns in enumerate(nsample):
        m, term = res["m"][q], res["term"][q]
        dm = (ns + 2) * eps * m + eps * L
        dterm = 2 * np.abs(m - L) / (L + 1e-8) * dm + dm ** 2 / (L + 1e-8) + 5 * eps * term
        bound += weight[q] * (dterm.mean() + (groups + len(percentage) + 3) * eps * term.mean())
    print(f"{kind} n={n}: restated {res['loss']:.9g} composed {got:.9g} diff {abs(got - res['loss']):.3g} "
          f"bound {bound:.3g}")
    assert abs(got - res["loss"]) <= bound
    # and the input holds padded, exactly full and truncated groups between the two clouds (the GPU tests
    # rely on it): a condition on the input
    kinds = set()
    for k2 in ("cube", "shell"):
        r2 = res if k2 == kind else U.uniform_restated(U.make_cloud(k2, 3, n, 100 + n), npoint, nsample, ball_radius,
                                                       weight, L)
        for q, ns in enumerate(nsample):
            h = r2["hits"][q]
            kinds |= {name for name, mask in (("padded", h < ns), ("full", h == ns), ("truncated", h > ns))
                      if mask.any()}
    assert kinds == {"padded", "full", "truncated"}


@pytest.mark.parametrize("kind", ["cube", "shell"])
@pytest.mark.parametrize("n,percentage", CASES[1:])
def test_restated_gradient_agrees_with_autograd(kind, n, percentage):
    xyz = U.make_cloud(kind, 2, n, 100 + n)
    b = xyz.shape[0]
    npoint, nsample, ball_radius, weight, L = U.uniform_params(n, percentage)
    res = U.uniform_restated(xyz, npoint, nsample, ball_radius, weight, L)
    grad, count, mag = U.uniform_gradient_f64(xyz, npoint, nsample, weight, L, res)
    assert count.max() > 1 and (count == 0).any()  # points in several slots, and points in none

    # float64 torch over the same index lists and neighbour slots.  u keeps the contract's float32 VALUE
    # (so m and the coefficient are the restatement's) and the float64 root's derivative.
    p = torch.from_numpy(xyz.astype(np.float64)).requires_grad_(True)
    total = 0.0
    for q, g in enumerate(res["groups"]):
        e, vstar = res["e"][q], res["vstar"][q]
        u32, _ = U.u_values(e)
        live = torch.from_numpy((e > 0) & np.isfinite(e))
        gi = torch.from_numpy(g.astype(np.int64))
        gj = torch.gather(gi, 2, torch.from_numpy(np.maximum(vstar, 0).astype(np.int64)))
        batch = torch.arange(b).view(b, 1, 1).expand_as(gi)
        diff = p[batch, gi] - p[batch, gj]
        sq = (diff * diff).sum(-1)
        root = torch.sqrt(torch.where(live, sq, torch.ones_like(sq)))  # a zero distance adds nothing
        root = torch.where(live, root, torch.zeros_like(root))
        u = root + (torch.from_numpy(u32.astype(np.float64)) - root).detach()
        m = u.sum(-1) / nsample[q]
        total = total + weight[q] * ((m - L) ** 2 / (L + 1e-8)).sum() / (b * npoint)
    assert abs(total.item() - res["loss"]) <= 1e-12 * abs(res["loss"])
    total.backward()
    # the restatement divides by the float32 root.  With eps = 2^-24: each float32 difference is within
    # eps, its square within 2 eps, and the three roundings of the pinned sum add 3 eps: 5 eps on the
    # distance, 2.5 eps on its root, and sqrtf's own rounding makes 3.5 eps < 2^-22
    err = np.abs(p.grad.numpy() - grad)
    print(f"{kind} n={n}: worst error / bound {np.max(err / np.maximum(2.0 ** -22 * mag, 1e-300)):.3g}")
    assert (err <= 2.0 ** -22 * mag).all()
    assert np.abs(grad).max() > 0
