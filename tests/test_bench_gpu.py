"""bench.py's plain run on a GPU: the lean result line and --dump-outputs.

A plain run (no --full) times its steps and reports the headline only; with
--dump-outputs it writes what the last timed step returned.  The dumped arrays
are checked bit for bit against the CPU oracle on the bench's own seeded
clouds, the same standard test_chamfer_gpu.py holds the one-launch step to.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

# everything a plain run leaves to --full
FULL_ONLY = ("roofline", "roofline_hbm", "roofline_executed", "two_launch", "icp", "reference_call",
             "training_call", "dense_fp16", "emd", "emd_training_call", "emd_training_call_uniform", "cpu_baseline")


def _run(capsys, *argv):
    bench.main(list(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's forward and backward on rank 0's seeded clouds (bench.ChamferStep)."""
    g = torch.Generator(device="cpu").manual_seed(bench.BENCH_SEED)
    a = torch.rand(bench.B, bench.N, 3, generator=g).numpy()
    c = torch.rand(bench.B, bench.M, 3, generator=g).numpy()
    d1, d2, i1, i2 = oracle.chamfer_forward(a, c)
    w1, w2 = np.float32(1.0 / (bench.B * bench.N)), np.float32(1.0 / (bench.B * bench.M))
    g1, g2 = oracle.chamfer_backward(a, c, np.full((bench.B, bench.N), w1, np.float32),
                                     np.full((bench.B, bench.M), w2, np.float32), i1, i2)
    return d1, d2, i1, i2, g1, g2


@pytest.mark.parametrize("steps", [3, 21])  # one graph of 3 steps; one 20-step graph + a one-step tail
def test_plain_run_dumps_the_last_step(cuda, reference, capsys, tmp_path, steps):
    out = _run(capsys, "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(tmp_path))
    assert out["steps"] == steps and out["ms_per_step"] > 0
    assert out["unit"] == "point-pairs/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] == pytest.approx(2 * bench.B * bench.N * bench.M / (out["ms_per_step"] * 1e-3))
    assert not [k for k in FULL_ONLY if k in out]
    assert "steady_replay_us" not in out["graph"]

    got = {name: np.load(tmp_path / (name + ".npy")) for name in bench.DUMP_NAMES}
    assert sorted(os.listdir(tmp_path)) == sorted(name + ".npy" for name in bench.DUMP_NAMES)
    assert all(a.dtype == np.float32 for a in got.values())

    d1, d2, i1, i2, g1, g2 = reference
    np.testing.assert_array_equal(got["idx1"], i1.astype(np.float32))
    np.testing.assert_array_equal(got["idx2"], i2.astype(np.float32))
    np.testing.assert_array_equal(got["dist1"].view(np.int32), d1.view(np.int32))
    np.testing.assert_array_equal(got["dist2"].view(np.int32), d2.view(np.int32))
    np.testing.assert_array_equal(got["grad_xyz1"].view(np.int32), g1.view(np.int32))
    np.testing.assert_array_equal(got["grad_xyz2"].view(np.int32), g2.view(np.int32))
    means = np.array([d1.astype(np.float64).mean(), d2.astype(np.float64).mean()])
    np.testing.assert_allclose(got["loss"][:2], means, rtol=2e-6)  # test_loss_grad_matches_oracle's bound
    assert got["loss"][2] == np.float32(got["loss"][0] + got["loss"][1])
