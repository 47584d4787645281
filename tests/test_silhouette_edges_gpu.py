"""csrc/silhouette.hip on the edges of its launch geometry: the cases of
tests/silhouette_restated.py (grids with one row or column and with partial
tiles and bands, point counts on the chunk, wave and workgroup splits, four
sigma_sq, six input families) against the float64 restatements within the
tolerances of tests/test_silhouette_gpu.py, which tests/test_silhouette_edges_cpu.py
shows to leave the float32 arithmetic a factor of four.  Every output is
pre-filled with a sentinel and must be fully overwritten; rows and planes give
the same bits; a cloud alone equals its place in the batch; a non-finite point
changes no other point's gradient; a grid of 129 is refused with nothing
written.

Every case keeps its largest error / tolerance; the last test prints the worst
per grid and per sigma_sq (with pcm_proj_bce's of tests/test_silhouette_gpu.py
when that ran earlier in the same process: name it first on the command line)
and writes them into the file PCM_EDGES_RECORD names (profiles/edges/ holds
such a record)."""
import os

import numpy as np
import pytest
import torch

import silhouette_restated as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0


def _forward(x, grid_h, grid_w, sigma_sq, out=None):
    import pcm_hip
    if out is None:
        out = torch.full((x.shape[0], grid_h, grid_w), SENTINEL, device=x.device)
    pcm_hip.silhouette_forward(x, pcm_hip.cloud_layout(x), grid_h, grid_w, sigma_sq, out)
    return out


def _backward(x, G, grid_h, grid_w, sigma_sq):
    """The gradient in the cloud's own layout, written over a sentinel."""
    import pcm_hip
    out = torch.full_like(x, SENTINEL)  # keeps the cloud's strides
    assert out.stride() == x.stride()
    pcm_hip.silhouette_backward(x, pcm_hip.cloud_layout(x), grid_h, grid_w, sigma_sq, G, out)
    return out


def _planes(x):
    """The same cloud as a [B, N, 3] view of contiguous [B, 3, N] planes."""
    return x.transpose(1, 2).contiguous().transpose(1, 2)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ratio(err, bound):
    return float(np.max(np.where(err == 0, 0.0, err / bound), initial=0.0))


def _layouts(xyz, cuda):
    import pcm_hip
    rows = torch.from_numpy(np.array(xyz)).to(cuda)
    planes = _planes(rows)
    if rows.shape[1] > 1:
        assert pcm_hip.cloud_layout(rows) == 0 and pcm_hip.cloud_layout(planes) == 1
    return rows, planes


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_forward_at_the_edges(cuda, case):
    h, w = case.grid
    xyz = R.cloud(case.family, case.grid, case.n)
    rows, planes = _layouts(xyz, cuda)
    out = _forward(rows, h, w, case.sigma_sq)
    assert not (out == SENTINEL).any() and torch.isfinite(out).all()
    want = R.sil_f64(xyz, h, w, case.sigma_sq)
    got = out.cpu().numpy().astype(np.float64)
    ratio = _ratio(np.abs(got - want), R.FWD_RTOL * np.abs(want) + R.FWD_ATOL)
    R.note("forward", case.grid, case.sigma_sq, ratio)
    print(f"{R.case_id(case)}: forward error / tolerance {ratio:.3g}")
    np.testing.assert_allclose(got, want, rtol=R.FWD_RTOL, atol=R.FWD_ATOL)
    assert _same_bits(out, _forward(planes, h, w, case.sigma_sq))
    alone = _forward(rows[1:2].contiguous(), h, w, case.sigma_sq)
    assert _same_bits(alone[0], out[1])


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.case_id)
def test_backward_at_the_edges(cuda, case):
    h, w = case.grid
    xyz = R.cloud(case.family, case.grid, case.n)
    G = R.grad_sil(case.grid, case.n)
    rows, planes = _layouts(xyz, cuda)
    Gd = torch.from_numpy(G).to(cuda)
    grad = _backward(rows, Gd, h, w, case.sigma_sq)
    assert not (grad == SENTINEL).any()
    assert (_bits(grad[..., 2]) == 0).all()  # exactly +0
    want, A = R.grad_f64(xyz, G, h, w, case.sigma_sq)
    got = grad.cpu().numpy().astype(np.float64)
    err = np.abs(got[..., :2] - want[..., :2])
    bound = R.backward_bound(h, w, A)
    ratio = _ratio(err, bound)
    R.note("backward", case.grid, case.sigma_sq, ratio)
    print(f"{R.case_id(case)}: backward error / bound {ratio:.3g}")
    assert (err <= bound).all()
    g_planes = _backward(planes, Gd, h, w, case.sigma_sq)
    assert g_planes.stride() == planes.stride() and not (g_planes == SENTINEL).any()
    assert _same_bits(grad, g_planes)


def test_backward_non_finite_point_leaves_every_other_point_alone(cuda):
    """Each thread reads only its own point (include/pcm.h: unspecified for that point; all other points are
    unaffected): 70 points at grid (33, 17) are two workgroups of 64 points and two slices, the NaN point in
    the first and the +inf point in the second, both in cloud 1."""
    h, w, n, s2 = 33, 17, 70, 0.5
    xyz = np.array(R.cloud("unit", (h, w), n))
    G = torch.from_numpy(R.grad_sil((h, w), n)).to(cuda)
    bad = xyz.copy()
    bad[1, 5, 0] = np.nan
    bad[1, 66, 1] = np.inf
    others = np.ones((R.B, n), bool)
    others[1, 5] = others[1, 66] = False
    for make in (lambda t: t, _planes):
        base = _backward(make(torch.from_numpy(xyz).to(cuda)), G, h, w, s2)
        got = _backward(make(torch.from_numpy(bad).to(cuda)), G, h, w, s2)
        assert not (got == SENTINEL).any()
        a, b = _bits(base).numpy(), _bits(got).numpy()
        assert np.array_equal(a[others], b[others])
        assert (b[..., 2] == 0).all()


@pytest.mark.parametrize("grid", [(129, 8), (8, 129), (129, 129)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_a_grid_above_the_limit_is_refused_with_nothing_written(cuda, grid):
    import pcm_hip
    assert pcm_hip.SILHOUETTE_MAX_GRID == 128
    h, w = grid
    x = torch.from_numpy(np.array(R.cloud("unit", (33, 31), 17))).to(cuda)
    out = torch.full((R.B, h, w), SENTINEL, device=cuda)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.silhouette_forward(x, 0, h, w, 0.5, out)
    grad = torch.full_like(x, SENTINEL)
    with pytest.raises(pcm_hip.PcmError):
        pcm_hip.silhouette_backward(x, 0, h, w, 0.5, torch.zeros(R.B, h, w, device=cuda), grad)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (grad == SENTINEL).all()


def test_a_grid_at_the_limit_passes(cuda):
    x = torch.from_numpy(np.array(R.cloud("unit", (33, 31), 17))).to(cuda)
    out = _forward(x, 128, 128, 0.5)
    want = R.sil_f64(x.cpu().numpy(), 128, 128, 0.5)
    np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), want, rtol=R.FWD_RTOL, atol=R.FWD_ATOL)
    G = torch.from_numpy(R.grad_sil((128, 128), 17)).to(cuda)
    grad = _backward(x, G, 128, 128, 0.5)
    ref, A = R.grad_f64(x.cpu().numpy(), G.cpu().numpy(), 128, 128, 0.5)
    assert (np.abs(grad.cpu().numpy()[..., :2] - ref[..., :2]) <= R.backward_bound(128, 128, A)).all()


def test_record_worst_ratio():
    """After the comparisons above (same process): the figures for profiles/edges/."""
    lines = []
    for kind, first, second in (("forward", "grid", "sigma_sq"), ("backward", "grid", "sigma_sq"),
                                ("bce", "count", "gt scale")):
        vals = {k[1:]: v for k, v in R.WORST.items() if k[0] == kind}
        if not vals:
            continue
        lines.append(f"{kind}: worst error / tolerance {max(vals.values()):.4g}")
        for name, pos in ((first, 0), (second, 1)):
            for key in sorted({k[pos] for k in vals}):
                worst = max(v for k, v in vals.items() if k[pos] == key)
                shown = "x".join(map(str, key)) if isinstance(key, tuple) else f"{key:g}"
                if isinstance(key, int):
                    shown = str(key)  # a count, in full
                lines.append(f"  {kind} {name} {shown}: {worst:.4g}")
    print("\n".join(lines))
    if os.environ.get("PCM_EDGES_RECORD") and lines:
        with open(os.path.join(REPO, os.environ["PCM_EDGES_RECORD"]), "w") as f:
            f.write(f"tests/test_silhouette_edges_gpu.py and pcm_proj_bce of tests/test_silhouette_gpu.py on "
                    f"{torch.cuda.get_device_name(0)}\nlargest error / tolerance:\n" + "\n".join(lines) + "\n")
