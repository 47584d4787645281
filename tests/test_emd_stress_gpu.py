"""The HIP EMD auction outside the unit cube and on degenerate geometry.

csrc/emd.hip skips work it proves irrelevant (the 64-entry cache's bound T, the
seed-time reserve's rT, the fast scan on float32 keys, bisection thresholds,
tail and chain modes).  A wrong bound does not crash: it changes a few
assignments, and only where the bound is tight.  Every other EMD test draws
both clouds from [0,1)^3; the inputs here (tests/emd_stress_cases.py) have
coordinates of magnitude 1e-4 to 1e5, common offsets, planar, collinear and
lattice clouds, coincident, collapsed, clustered and bimodal clouds and a far
outlier.  tests/test_emd_stress_cpu.py keeps the oracle honest on them.

  * parity: the plain entry must equal the oracle in assignment, dist bits and
    price bits, at 300 iterations and at the converge length of 3000;
  * the tuning entries (no helpers, all helpers, no tail mode, always tail
    mode) must give the same bits; their counters are printed (run with -s),
    not asserted;
  * the auction's guarantee, checked on the GPU result without the oracle --
    what still fails if the kernels and the oracle were wrong together;
  * backward and the Loss module on shifted and scaled clouds.
"""
import functools

import numpy as np
import pytest
import torch

import emd_stress_cases as S
from emd_optimality_check import check_eps_optimal
from reference_cases import bits, graddist

pytestmark = pytest.mark.gpu

_PARITY = ([(name, n, iters) for name, n in S.ENTRIES for iters in (S.SHORT_ITERS, S.CONVERGE_ITERS)]
           + [S.LARGE])
_TUNED_CASES = ("scale_1e-4", "scale_1e3", "lattice_half_shift", "collapsed_targets")
# as tests/test_emd_gpu.py::test_emd_helper_configs_match_oracle
_CONFIGS = {"no_helpers": dict(helpers=0), "all_helpers": dict(helpers=31, offload_min=0),
            "no_tail": dict(tail_max=0), "all_tail": dict(tail_max=1024)}


def _run_id(run):
    return f"{run[0]}-n{run[1]}-it{run[2]}"


@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, name, n, iters):
    a, c, eps = S.clouds(name, n)
    dist, ass, price, _ = oracle.emd_forward(a, c, eps, iters, with_stats=True)
    return dist, ass, price


def _forward(a, c, eps, iters, dev, **tuning):
    import pcm_hip
    b, n, _ = a.shape
    dist = torch.full((b, n), float("nan"), device=dev)
    ass = torch.full((b, n), -7, dtype=torch.int32, device=dev)
    price = torch.full((b, n), float("nan"), device=dev)
    pcm_hip.emd_forward(torch.from_numpy(a).to(dev), torch.from_numpy(c).to(dev), eps, iters, dist, ass, price,
                        **tuning)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), ass.cpu().numpy(), price.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gpu_run(dev, name, n, iters):
    """The product path: pcm_hip.emd_forward with no tuning argument."""
    a, c, eps = S.clouds(name, n)
    return _forward(a, c, eps, iters, dev)


def _assert_same_bits(got, want):
    (dist, ass, price), (rd, ra, rp) = got, want
    differ = int((ass != ra).sum())
    assert differ == 0, f"{differ} of {ass.size} assignments differ from the oracle's"
    np.testing.assert_array_equal(bits(dist), bits(rd))
    np.testing.assert_array_equal(bits(price), bits(rp))


@pytest.mark.parametrize("run", _PARITY, ids=_run_id)
def test_emd_forward_matches_oracle(cuda, oracle, run):
    name, n, iters = run
    a, c, _ = S.clouds(name, n)
    dist, ass, price = _gpu_run(cuda, name, n, iters)
    assert ((ass >= 0) & (ass < n)).all()
    # the reference's "Verified EMD" (metric/emd/test.py:24-28) in float64
    dif = a.astype(np.float64) - np.take_along_axis(c, ass[..., None].astype(np.int64), axis=1)
    np.testing.assert_allclose(dist, (dif * dif).sum(-1), rtol=1e-6, atol=0)
    _assert_same_bits((dist, ass, price), _oracle_run(oracle, name, n, iters))


@pytest.mark.parametrize("config", sorted(_CONFIGS))
@pytest.mark.parametrize("name", _TUNED_CASES)
def test_emd_tuning_entries_match_oracle(cuda, oracle, name, config):
    n, iters = 1024, S.SHORT_ITERS
    a, c, eps = S.clouds(name, n)
    stats = torch.zeros(3 * iters + 16 + 1, dtype=torch.int32, device=cuda)
    got = _forward(a, c, eps, iters, cuda, stats=stats, **_CONFIGS[config])
    st = stats.cpu().numpy()
    # nobody has measured these at such ranges: reported, not asserted
    print(f"\n{name:20s}{config:12s}bidders {int(st[0:2 * iters:2].sum()):<7d}full scans "
          f"{int(st[1:2 * iters:2].sum()):<7d}jobs {st[2 * iters + 10]:<6d}reserve bids {st[2 * iters + 13]}")
    _assert_same_bits(got, _oracle_run(oracle, name, n, iters))


@pytest.mark.parametrize("entry", S.CONVERGING, ids=S.entry_id)
def test_emd_forward_is_eps_optimal(cuda, entry):
    """Bijection, eps-complementary slackness within 4 float32 ulps of the
    case's magnitude, and (n <= 2048) cost within n * (eps + slack) of the
    exact optimum: no oracle involved."""
    name, n = entry
    a, c, eps = S.clouds(name, n)
    _, ass, price = _gpu_run(cuda, name, n, S.CONVERGE_ITERS)
    r = check_eps_optimal(a[0], c[0], ass[0], price[0], eps, solve=n <= 2048)
    print(f"\n{name:22s}n={n:<6d}(gap-eps)/ulp(M)={(r.worst_gap - eps) / (2.0 ** -24 * r.magnitude):+.2f}"
          f"  excess/(n eps)={'-' if r.excess is None else format(r.excess, '.3f')}")


@pytest.mark.parametrize("name", ["scale_1e3", "centred"])
def test_emd_backward_matches_oracle(cuda, oracle, name):
    import pcm_hip
    b, n = 2, 1024
    a, c, eps = S.clouds(name, n, b=b)
    _, ass = oracle.emd_forward(a, c, eps, S.SHORT_ITERS)
    gd = graddist(500, b, n)
    grad = torch.full((b, n, 3), float("nan"), device=cuda)
    pcm_hip.emd_backward(torch.from_numpy(a).to(cuda), torch.from_numpy(c).to(cuda), torch.from_numpy(gd).to(cuda),
                         torch.from_numpy(ass).to(cuda), grad)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(grad.cpu().numpy()), bits(oracle.emd_backward(a, c, gd, ass)))


def test_emd_loss_on_centred_clouds(cuda, oracle):
    # loss/loss.py:22-25 at its defaults (eps 0.05, 3000 iterations), as
    # tests/test_emd_gpu.py::test_emd_loss_like_reference
    import loss
    a, c, eps = S.clouds("centred", 1024)
    assert eps == 0.05
    got = loss.Loss().get_emd_loss(torch.from_numpy(a).to(cuda), torch.from_numpy(c).to(cuda)).item()
    rd = _oracle_run(oracle, "centred", 1024, S.CONVERGE_ITERS)[0]
    assert abs(got - float(np.sqrt(rd.astype(np.float64)).mean())) < 1e-6
