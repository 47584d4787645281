"""Pins oracle/pcm_oracle.c to the REFERENCE's own kernels, on the CPU.

oracle/ref_build.py compiles the reference's chamfer3D.cu and emd_cuda.cu for
the host (threads as fibers, -ffp-contract=off).  That build evaluates
x*x+y*y+z*z unfused, so the oracle is run at order=1 (unfused) wherever a
squared distance is involved and must then equal it BIT FOR BIT: tile and tie
order, the GetMax window, the double arithmetic of the bid value, the NaN
rules and the order of the backward's adds are then the reference's own.
Which FMA contraction nvcc picks is NOT pinned by this (nor can it be here).

Schedules: the emulator runs blocks and threads ascending or descending.  The
oracle's deterministic GetMax rule (lowest bidder wins) is the reference under
the DESCENDING schedule; the cases marked race-free give the same result under
both, so there the reference's output does not depend on the race at all.

Skipped only where the reference directory is absent (the GPU machines).
Observed timings in the emulator (one schedule): 1.9 s, 4.0 s, 4.9 s, 3.9 s
for the four EMD cases, 0.5 s per Chamfer forward, milliseconds per backward.
"""
import functools

import numpy as np
import pytest

import ref_build
import reference_cases as C
from reference_cases import bits

needs_reference = pytest.mark.skipif(not ref_build.available(),
                                     reason="reference directory absent (PCM_REFERENCE)")


@functools.lru_cache(maxsize=None)
def _emd_inputs(name):
    return C.EMD_CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _ref_emd(name, descending):
    a, c = _emd_inputs(name)
    _, eps, iters, _, _ = C.EMD_CASES[name]
    return ref_build.ref_emd_forward(a, c, eps, iters, descending)


@functools.lru_cache(maxsize=None)
def _ref_chamfer(name):
    a, c = C.CHAMFER_FORWARD_CASES[name]()
    return a, c, ref_build.ref_chamfer_forward(a, c)


def test_launch_rewrite_touches_only_the_launch():
    text = "k<<<dim3(b, n / 1024, 1), 1024>>>(b, n,\n\tp.data<int>());\nint x = a < b;"
    assert ref_build.rewrite_launches(text) == (
        "CUDA_ON_CPU_LAUNCH(k, dim3(b, n / 1024, 1), 1024)(b, n,\n\tp.data<int>());\nint x = a < b;")
    with pytest.raises(RuntimeError):
        ref_build.rewrite_launches("int main() { return 0; }")


@needs_reference
@pytest.mark.parametrize("name", sorted(C.EMD_CASES))
def test_emd_forward_oracle_equals_reference_descending(oracle, name):
    """Assignment and dist bitwise on every case.  Price is compared, in full,
    only on the converged case: on the others the reference's last iteration
    does `price +=` for every remaining bidder (a race the oracle deliberately
    leaves out), so price is left out there altogether."""
    a, c = _emd_inputs(name)
    _, eps, iters, _, converged = C.EMD_CASES[name]
    rd, ra, rp = _ref_emd(name, True)
    od, oa, op, hist = oracle.emd_forward(a, c, eps, iters, with_stats=True, order=1)
    np.testing.assert_array_equal(oa, ra)
    np.testing.assert_array_equal(bits(od), bits(rd))
    assert (hist[-1] == 0) == converged
    if converged:
        np.testing.assert_array_equal(bits(op), bits(rp))
    # the shipped evaluation order (what the HIP kernels compute) assigns alike
    _, oa0 = oracle.emd_forward(a, c, eps, iters)
    np.testing.assert_array_equal(oa0, ra)


@needs_reference
@pytest.mark.parametrize("name", sorted(k for k, v in C.EMD_CASES.items() if v[3]))
def test_emd_forward_race_free_cases_ignore_the_schedule(name):
    """A case that fails here is racy in the reference: replace it."""
    for got, want in zip(_ref_emd(name, False), _ref_emd(name, True)):
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


@needs_reference
def test_emd_racy_cases_do_depend_on_the_schedule():
    # the N > 2048 cases are where GetMax's last-writer race decides; if they
    # stopped depending on it the descending pin above would prove less
    name = "exact_ties_n4096"
    assert (_ref_emd(name, False)[1] != _ref_emd(name, True)[1]).any()


@needs_reference
@pytest.mark.parametrize("name", sorted(C.CHAMFER_FORWARD_CASES))
def test_chamfer_forward_oracle_equals_reference(oracle, name):
    a, c, (d1, d2, i1, i2) = _ref_chamfer(name)
    o1, j1 = oracle.chamfer_nn(a, c, order=1)
    o2, j2 = oracle.chamfer_nn(c, a, order=1)
    np.testing.assert_array_equal(j1, i1)
    np.testing.assert_array_equal(j2, i2)
    np.testing.assert_array_equal(np.isnan(o1), np.isnan(d1))
    np.testing.assert_array_equal(np.isnan(o2), np.isnan(d2))
    np.testing.assert_array_equal(bits(o1), bits(d1))
    np.testing.assert_array_equal(bits(o2), bits(d2))
    # the shipped order picks the same neighbours on these clouds
    _, _, s1, s2 = oracle.chamfer_forward(a, c)
    np.testing.assert_array_equal(s1, i1)
    np.testing.assert_array_equal(s2, i2)


@needs_reference
def test_chamfer_nan_cases_hold_what_they_claim():
    _, _, (d1, d2, i1, _) = _ref_chamfer("nan_tiles_700x1300")
    assert np.isnan(d1).all() and (i1 == 0).all()          # NaN at target 0 poisons tile 0
    assert np.isnan(d2).sum() == 2 * 3 and np.isinf(d2[:, 700]).all()
    a, c, (d1, _, i1, _) = _ref_chamfer("nan_tile3_300x1600")
    assert np.isnan(c[0, 1536]).any() and not np.isnan(d1).any() and (i1 < 1536).all()


@needs_reference
def test_committed_fixture_is_what_the_reference_computes():
    """tests/golden/ref_kernels_golden.npz (the GPU suite's yardstick) against a
    fresh run of the reference's kernels: inputs and outputs, every recorded case."""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kernels_golden.npz"))
    for name in gold["emd_cases"]:
        a, c = _emd_inputs(str(name))
        dist, ass, _ = _ref_emd(str(name), True)
        _, eps, iters, _, _ = C.EMD_CASES[str(name)]
        assert float(gold[f"emd/{name}/eps"]) == np.float32(eps) and int(gold[f"emd/{name}/iters"]) == iters
        for key, want in (("xyz1", a), ("xyz2", c), ("dist", dist)):
            np.testing.assert_array_equal(bits(gold[f"emd/{name}/{key}"]), bits(want))
        np.testing.assert_array_equal(gold[f"emd/{name}/assignment"], ass)
        if f"emd/{name}/gradxyz1" in gold.files:
            grad = ref_build.ref_emd_backward(a, c, gold[f"emd/{name}/graddist"], ass)
            np.testing.assert_array_equal(bits(gold[f"emd/{name}/gradxyz1"]), bits(grad))
    for name in gold["chamfer_cases"]:
        a, c, (d1, d2, i1, i2) = _ref_chamfer(str(name))
        for key, want in (("xyz1", a), ("xyz2", c), ("dist1", d1), ("dist2", d2)):
            np.testing.assert_array_equal(bits(gold[f"chamfer/{name}/{key}"]), bits(want))
        np.testing.assert_array_equal(gold[f"chamfer/{name}/idx1"], i1)
        np.testing.assert_array_equal(gold[f"chamfer/{name}/idx2"], i2)
        if f"chamfer/{name}/gradxyz1" in gold.files:
            g1, g2 = ref_build.ref_chamfer_backward(a, c, gold[f"chamfer/{name}/graddist1"],
                                                    gold[f"chamfer/{name}/graddist2"], i1, i2)
            np.testing.assert_array_equal(bits(gold[f"chamfer/{name}/gradxyz1"]), bits(g1))
            np.testing.assert_array_equal(bits(gold[f"chamfer/{name}/gradxyz2"]), bits(g2))


@needs_reference
@pytest.mark.parametrize("b,n,m,seed", [(2, 700, 1300, 60), (1, 4096, 257, 61), (1, 300, 4096, 62)])
def test_chamfer_backward_oracle_equals_reference(oracle, b, n, m, seed):
    """g*(x1-x2) has nothing to contract, so the shipped oracle must equal the
    ascending-schedule reference bit for bit while n, m <= 4096 (one point per
    thread of the 16 x 256 grid, chamfer3D.cu:157,184: adds land in ascending
    point order, kernel 1 before kernel 2)."""
    a, c = C.chamfer_clouds(seed, b, n, m)
    _, _, i1, i2 = oracle.chamfer_forward(a, c)
    assert np.bincount(i1[0], minlength=m).max() > 1       # several scatter terms per point
    gd1, gd2 = C.graddist(seed + 100, b, n), C.graddist(seed + 200, b, m)
    r1, r2 = ref_build.ref_chamfer_backward(a, c, gd1, gd2, i1, i2)
    o1, o2 = oracle.chamfer_backward(a, c, gd1, gd2, i1, i2)
    np.testing.assert_array_equal(bits(o1), bits(r1))
    np.testing.assert_array_equal(bits(o2), bits(r2))


@needs_reference
def test_chamfer_backward_add_order_changes_above_4096(oracle):
    """Above 4096 points the grid-stride loop (chamfer3D.cu:157) makes thread t
    add points t, t+4096, ... before thread t+1 starts, so the ascending
    schedule is no longer ascending point order; the reference's order there is
    the hardware's choice and stays unpinned.  Only ordering differs: the sums
    agree to rounding."""
    b, n, m = 1, 5000, 300
    a, c = C.chamfer_clouds(63, b, n, m)
    _, _, i1, i2 = oracle.chamfer_forward(a, c)
    gd1, gd2 = C.graddist(163, b, n), C.graddist(263, b, m)
    r1, r2 = ref_build.ref_chamfer_backward(a, c, gd1, gd2, i1, i2)
    o1, o2 = oracle.chamfer_backward(a, c, gd1, gd2, i1, i2)
    np.testing.assert_array_equal(bits(o1), bits(r1))      # one scatter source per kernel-2 thread still
    assert (bits(o2) != bits(r2)).any()
    # both sides add the same float32 terms t, in different orders: each sum of
    # k terms is within (k-1) * 2^-24 * sum|t| of the exact one (to first order)
    f64 = np.float64
    t_abs = np.zeros((m, 3))
    np.add.at(t_abs, i1[0], np.abs(2 * gd1[0][:, None].astype(f64) * (a[0].astype(f64) - c[0][i1[0]])))
    t_abs += np.abs(2 * gd2[0][:, None].astype(f64) * (c[0].astype(f64) - a[0][i2[0]]))
    k = np.bincount(i1[0], minlength=m).max() + 1
    assert (np.abs(o2[0].astype(f64) - r2[0]) <= 2 * k * 2.0 ** -24 * t_abs).all()


@needs_reference
@pytest.mark.parametrize("b,n,seed", [(2, 1024, 70), (1, 4096, 71), (1, 8192, 72)])
def test_emd_backward_oracle_equals_reference(oracle, b, n, seed):
    """One add per point into a zero-filled gradient (emd_cuda.cu:284-300): the
    order cannot matter, at any n."""
    g = np.random.default_rng(seed)
    a, c = C.uniform_clouds(seed, b, n)
    ass = np.stack([g.permutation(n) for _ in range(b)]).astype(np.int32)
    gd = C.graddist(seed + 100, b, n)
    for descending in (False, True):
        r = ref_build.ref_emd_backward(a, c, gd, ass, descending)
        np.testing.assert_array_equal(bits(oracle.emd_backward(a, c, gd, ass)), bits(r))
