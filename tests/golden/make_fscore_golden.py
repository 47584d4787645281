#!/usr/bin/env python3
"""Generate the committed F-score golden fixture from the REFERENCE's own code.

Runs only where the reference tree exists (never on the GPU box).  It loads
the reference's ``loss/loss_.py`` and evaluates its ``batch_NN_loss`` (:93-109,
float64 distance matrix) and ``fscore`` (:122-140) on CPU tensors.  That file
imports geomloss and the CUDA Chamfer extension at module scope (:2, :7),
neither of which fscore uses, so two empty stub modules of our own stand in
for them while it loads (and are removed again).

Per case the fixture holds the clouds and, for every threshold,
  count_x [B,T]   (mins2 < th).sum(1): points of X within th of Y (mins2 is
                  the reference's per-X-point distance)
  count_y [B,T]   (mins1 < th).sum(1): points of Y within th of X
  per_cloud [B,T,3]  the reference's fscore(X[i:i+1], Y[i:i+1], th) triple
                  (fscore, precision_1 = share of Y, precision_2 = share of X)
  batch [T,3]     the reference's fscore(X, Y, th) triple on the whole batch
Noisy cases are c = a[random points] + 0.01 randn -- a prediction scattered
around its ground truth, the regime the metric is used in; uniform cases are
two independent torch.rand clouds.

The generator ASSERTS that no reference float64 distance lies within a
relative 1e-5 of any threshold -- about 100x the rounding of the float32
pinned expression fma(dz,dz,fma(dy,dy,dx*dx)) -- so a float32 path's counts
must equal the reference's exactly.  A case that fails is replaced by another
seed, never tolerated.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fscore_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("PCM_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fscore_golden.npz")

THRESHOLDS = (1e-4, 2.5e-4, 1e-3, 1e-2)
MARGIN = 1e-5
CASES = [  # (name, seed, kind, B, N, M)
    ("noisy_256", 0, "noisy", 4, 256, 256),
    ("noisy_ragged", 1, "noisy", 2, 200, 300),
    ("noisy_1024", 2, "noisy", 3, 1024, 1024),
    ("uniform_test_py", 3, "uniform", 2, 1000, 2000),
    ("noisy_64_2500", 4, "noisy", 1, 64, 2500),
    ("uniform_256", 5, "uniform", 2, 256, 256),
]


def reference_available():
    return os.path.exists(os.path.join(REF, "loss", "loss_.py"))


def load_reference():
    """The reference's loss/loss_.py as a module of its own name space."""
    sys.dont_write_bytecode = True
    stubs = {"geomloss": types.ModuleType("geomloss"), "dist_chamfer_3D": types.ModuleType("dist_chamfer_3D")}
    stubs["geomloss"].SamplesLoss = None
    stubs["dist_chamfer_3D"].chamfer_3DDist = None
    saved = {k: sys.modules.get(k) for k in stubs}
    saved_path = list(sys.path)
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_reference_loss_", os.path.join(REF, "loss", "loss_.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        sys.path[:] = saved_path
    return mod


def clouds(seed, kind, b, n, m):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(b, n, 3, generator=g)
    if kind == "uniform":
        return a, torch.rand(b, m, 3, generator=g)
    pick = torch.randint(0, n, (b, m), generator=g)
    c = torch.gather(a, 1, pick[:, :, None].expand(b, m, 3)) + 0.01 * torch.randn(b, m, 3, generator=g)
    return a, c.contiguous()


def generate(ref=None):
    ref = ref or load_reference()
    out = {}
    worst = float("inf")
    for name, seed, kind, b, n, m in CASES:
        a, c = clouds(seed, kind, b, n, m)
        _, mins1, mins2 = ref.batch_NN_loss(a, c)  # float64: per-Y-point, per-X-point
        assert mins1.dtype == torch.float64 and tuple(mins1.shape) == (b, m) and tuple(mins2.shape) == (b, n)
        count_x = np.zeros((b, len(THRESHOLDS)), np.int32)
        count_y = np.zeros((b, len(THRESHOLDS)), np.int32)
        per_cloud = np.zeros((b, len(THRESHOLDS), 3), np.float32)
        batch = np.zeros((len(THRESHOLDS), 3), np.float32)
        for t, th in enumerate(THRESHOLDS):
            for mins in (mins1, mins2):
                margin = float((torch.abs(mins - th) / th).min())
                worst = min(worst, margin)
                assert margin > MARGIN, (
                    f"{name}: a reference distance lies within {margin:.3g} (relative) of threshold {th}; "
                    "replace the case's seed")
            count_y[:, t] = (mins1 < th).sum(1).numpy()
            count_x[:, t] = (mins2 < th).sum(1).numpy()
            for i in range(b):
                per_cloud[i, t] = [float(v.detach()) for v in ref.fscore(a[i:i + 1], c[i:i + 1], th)]
            batch[t] = [float(v.detach()) for v in ref.fscore(a, c, th)]
        out[f"{name}/xyz1"] = a.numpy()
        out[f"{name}/xyz2"] = c.numpy()
        out[f"{name}/count_x"] = count_x
        out[f"{name}/count_y"] = count_y
        out[f"{name}/per_cloud"] = per_cloud
        out[f"{name}/batch"] = batch
        print(f"{name}: B={b} N={n} M={m} count_x[0]={count_x[0].tolist()} batch f={batch[:, 0].tolist()}")
    out["cases"] = np.array([c[0] for c in CASES])
    out["thresholds"] = np.array(THRESHOLDS, np.float64)
    print(f"smallest relative margin between a reference distance and a threshold: {worst:.3g}")
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
