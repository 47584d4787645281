#!/usr/bin/env python3
"""Generate the committed farthest-point-sampling fixture from the REFERENCE's own code.

Runs only where the reference tree exists (never on the GPU box).  It loads
the reference's ``utils/utils.py`` by path, with the reference's ``loss/`` and
``utils/`` in front of ``sys.path`` while it loads so that its own imports
(``proj_loss``, ``projection``) resolve to the reference's files, and evaluates
its ``farthest_point_sample`` (:335-360) on CPU tensors.

Per case the fixture holds
  <name>/xyz     [B, N, 3] float32  the cloud, ``torch.rand`` from a seeded
                 torch.Generator (``dups``: a 64-point cloud twice, so every
                 tie is exact; ``nonfinite``: a NaN, a +inf and a -inf)
  <name>/idx     [B, S] int64       the reference's farthest_point_sample(xyz, S, RAN)
  <name>/npoint  S,  <name>/ran  RAN

A condition, not a measurement: the generator also runs a numpy restatement of
pcm_fps's contract (include/pcm.h: the pinned fma order, strict '<', lowest
index on ties) and asserts, for every pick that is used, that the restatement
equals the reference exactly and that the winner beats the runner-up by a
relative margin of at least MARGIN, or ties it exactly.  1e-6 is about 8
float32 ulps; two distances computed in different summation orders differ by a
couple, so every correctly rounded order picks the same indices and exact
equality is a fair demand on the kernel.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fps_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("PCM_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fps_golden.npz")
MARGIN = 1e-6

CASES = [  # (name, seed, B, N, S, RAN)
    ("train128", 0, 2, 1024, 128, False),
    ("train256", 0, 2, 1024, 256, True),
    ("ragged", 1, 3, 300, 77, True),
    ("odd", 2, 2, 65, 65, False),
    ("two_chunks", 3, 1, 2053, 300, True),
    ("dups", 4, 1, 128, 100, True),
    ("tiny", 5, 2, 2, 2, False),
    ("oversample", 6, 1, 5, 8, True),
    ("nonfinite", 7, 1, 16, 10, True),
]


def reference_available():
    return os.path.exists(os.path.join(REF, "utils", "utils.py"))


def load_reference():
    """The reference's utils/utils.py as a module of its own name space; the
    modules it imports by bare name are the reference's, and whatever those
    names meant to the caller before is put back."""
    sys.dont_write_bytecode = True
    names = ("proj_loss", "projection")
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    path = list(sys.path)
    sys.path[:0] = [os.path.join(REF, "loss"), os.path.join(REF, "utils")]
    try:
        spec = importlib.util.spec_from_file_location("_reference_utils", os.path.join(REF, "utils", "utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = path
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    return mod


def cloud(name, seed, b, n):
    g = torch.Generator().manual_seed(seed)
    if name == "dups":
        half = torch.rand(b, n // 2, 3, generator=g)
        return torch.cat([half, half], 1)
    xyz = torch.rand(b, n, 3, generator=g)
    if name == "nonfinite":
        xyz[0, 3, 1] = float("nan")
        xyz[0, 9, 0] = float("inf")
        xyz[0, 12, 2] = float("-inf")
    return xyz


def sqd_pinned(d):
    """fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on float32 rows [n, 3]: each fused
    step is formed in float64 (the product is exact there) and rounded once."""
    dx, dy, dz = (d[:, c].astype(np.float32) for c in range(3))
    t = (dx * dx).astype(np.float32)
    t = (dy.astype(np.float64) * dy + t).astype(np.float32)
    return (dz.astype(np.float64) * dz + t).astype(np.float32)


def fps_restated(xyz, npoint, start):
    """pcm_fps's contract in numpy: idx [B, npoint] int64 and the smallest
    relative margin between a used pick's winner and a runner-up it does not
    tie exactly (inf if there is none)."""
    b, n, _ = xyz.shape
    idx = np.zeros((b, npoint), np.int64)
    worst = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        for bi in range(b):
            p = xyz[bi]
            run = np.full(n, 1e10, np.float32)
            far = start
            for i in range(npoint):
                idx[bi, i] = far
                d = sqd_pinned(p - p[far])
                upd = d < run  # False for a NaN distance
                run[upd] = d[upd]
                far = int(np.argmax(run))  # the lowest index attaining the maximum
                if i + 1 < npoint:
                    v1 = run[far]
                    below = run[run != v1]  # exact ties aside: the next distinct value
                    if below.size:
                        worst = min(worst, float((np.float64(v1) - below.max()) / v1))
    return idx, worst


def generate(ref=None):
    ref = ref or load_reference()
    out = {}
    for name, seed, b, n, s, ran in CASES:
        xyz = cloud(name, seed, b, n)
        idx = ref.farthest_point_sample(xyz, s, RAN=ran)
        assert idx.dtype == torch.long and tuple(idx.shape) == (b, s)
        idx = idx.numpy().astype(np.int64)
        mine, worst = fps_restated(xyz.numpy(), s, 0 if ran else 1)
        assert np.array_equal(mine, idx), f"{name}: the restatement differs from the reference"
        assert worst >= MARGIN, f"{name}: a pick is decided by a margin of {worst:.3g}"
        out[f"{name}/xyz"] = xyz.numpy()
        out[f"{name}/idx"] = idx
        out[f"{name}/npoint"] = np.int64(s)
        out[f"{name}/ran"] = np.bool_(ran)
        print(f"{name}: B={b} N={n} S={s} RAN={ran} worst margin {worst:.3g} first {idx[0, :6].tolist()}")
    out["cases"] = np.array([c[0] for c in CASES])
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
