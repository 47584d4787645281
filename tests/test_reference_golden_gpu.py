"""HIP kernels against outputs recorded from the REFERENCE's own kernels.

tests/golden/ref_kernels_golden.npz holds inputs and the outputs of the
reference's chamfer3D.cu / emd_cuda.cu, compiled for the host with
-ffp-contract=off (tests/golden/make_ref_kernels_golden.py).  Unlike every other
parity test here, nothing in the expected values went through pcm_oracle.c.

Indices and assignments must be EQUAL (the maker records a case only when the
contraction cannot change them).  Distances differ by the contraction alone:
x*x+y*y+z*z has three roundings in any evaluation order, each at most 2^-24 of
a partial sum that is <= the result (all terms are non-negative), so two orders
differ by at most 6 * 2^-24 * ref.  NaN masks must be equal; an infinite
distance must be the same infinity.  g*(x1-x2) has nothing to contract and the
recorded clouds have <= 4096 points, where the reference's adds land in
ascending point order (tests/test_oracle_reference_cpu.py): gradients are
compared bit for bit.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels_golden.npz")
_GOLD = np.load(_PATH)
EMD_CASES = [str(s) for s in _GOLD["emd_cases"]]
CHAMFER_CASES = [str(s) for s in _GOLD["chamfer_cases"]]
REL = 6 * 2.0 ** -24


def _dev(x, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(cuda).contiguous()


def _assert_dist(got, ref):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    inf = np.isinf(ref)
    np.testing.assert_array_equal(got[inf], ref[inf])
    fin = np.isfinite(ref)
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64))
    bound = REL * ref[fin].astype(np.float64)
    worst = float((err - bound).max()) if fin.any() else 0.0
    assert (err <= bound).all(), f"dist off the reference by {worst:.3e} beyond 6*2^-24*ref"


@pytest.mark.parametrize("name", EMD_CASES)
def test_emd_forward_matches_reference_kernels(cuda, name):
    import pcm_hip
    g = lambda k: _GOLD[f"emd/{name}/{k}"]  # noqa: E731
    a, c = g("xyz1"), g("xyz2")
    b, n, _ = a.shape
    dist = torch.empty(b, n, device=cuda)
    ass = torch.empty(b, n, dtype=torch.int32, device=cuda)
    pcm_hip.emd_forward(_dev(a, cuda), _dev(c, cuda), float(g("eps")), int(g("iters")), dist, ass)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ass.cpu().numpy(), g("assignment").astype(np.int32))
    _assert_dist(dist.cpu().numpy(), g("dist"))


def test_emd_backward_matches_reference_kernels(cuda):
    import pcm_hip
    name = next(n for n in EMD_CASES if f"emd/{n}/gradxyz1" in _GOLD.files)
    g = lambda k: _GOLD[f"emd/{name}/{k}"]  # noqa: E731
    a = g("xyz1")
    grad = torch.full(a.shape, float("nan"), device=cuda)
    pcm_hip.emd_backward(_dev(a, cuda), _dev(g("xyz2"), cuda), _dev(g("graddist"), cuda),
                         _dev(g("assignment"), cuda, torch.int32), grad)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(grad.cpu().numpy().view(np.int32), g("gradxyz1").view(np.int32))


@pytest.mark.parametrize("name", CHAMFER_CASES)
def test_chamfer_forward_matches_reference_kernels(cuda, name):
    import pcm_hip
    g = lambda k: _GOLD[f"chamfer/{name}/{k}"]  # noqa: E731
    a, c = g("xyz1"), g("xyz2")
    b, n, _ = a.shape
    m = c.shape[1]
    d1 = torch.zeros(b, n, device=cuda)
    d2 = torch.zeros(b, m, device=cuda)
    i1 = torch.zeros(b, n, dtype=torch.int32, device=cuda)
    i2 = torch.zeros(b, m, dtype=torch.int32, device=cuda)
    pcm_hip.chamfer_forward(_dev(a, cuda), _dev(c, cuda), d1, d2, i1, i2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(i1.cpu().numpy(), g("idx1").astype(np.int32))
    np.testing.assert_array_equal(i2.cpu().numpy(), g("idx2").astype(np.int32))
    _assert_dist(d1.cpu().numpy(), g("dist1"))
    _assert_dist(d2.cpu().numpy(), g("dist2"))


def test_chamfer_backward_matches_reference_kernels(cuda):
    import pcm_hip
    name = next(n for n in CHAMFER_CASES if f"chamfer/{n}/gradxyz1" in _GOLD.files)
    g = lambda k: _GOLD[f"chamfer/{name}/{k}"]  # noqa: E731
    a, c = g("xyz1"), g("xyz2")
    g1 = torch.full(a.shape, float("nan"), device=cuda)
    g2 = torch.full(c.shape, float("nan"), device=cuda)
    pcm_hip.chamfer_backward(_dev(a, cuda), _dev(c, cuda), _dev(g("graddist1"), cuda), _dev(g("graddist2"), cuda),
                             _dev(g("idx1"), cuda, torch.int32), _dev(g("idx2"), cuda, torch.int32), g1, g2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g1.cpu().numpy().view(np.int32), g("gradxyz1").view(np.int32))
    np.testing.assert_array_equal(g2.cpu().numpy().view(np.int32), g("gradxyz2").view(np.int32))
