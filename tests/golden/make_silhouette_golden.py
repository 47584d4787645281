#!/usr/bin/env python3
"""Generate the committed silhouette golden fixture from the REFERENCE's own code.

Runs only where the reference tree exists (never on the GPU box).  It loads
the reference's ``utils/projection.py`` by path (it imports torch and numpy
only) and evaluates its ``cont_proj`` (:4-67) and ``perspective_transform``
(:110-146) on CPU tensors with ``device='cpu'``.  The reference's
``world2cam`` and ``get_loss_proj`` end in ``.cuda()`` and cannot run without a
device; the tests check those against float64 restatements of their own.

Per case the fixture holds
  <name>/xyz   [B, N, 3] float32   the cloud, ``rand * 2 - 1`` from a seeded
               torch.Generator (``far``: ``rand * 6 - 3``, so most of its
               terms underflow)
  <name>/sil   [B, H, W] float32   the reference's cont_proj(xyz, H, W, 'cpu', sigma_sq)
and, for one cloud in front of the camera (the ``ragged`` cloud with z + 2.5),
  persp/xyz, persp/out             perspective_transform's input and output.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_silhouette_golden.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("PCM_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "silhouette_golden.npz")

CASES = [  # (name, seed, B, N, H, W, sigma_sq, coordinate half-range)
    ("finetune", 0, 2, 1024, 64, 64, 2.0, 1.0),
    ("ragged", 1, 3, 300, 16, 24, 2.0, 1.0),
    ("one_point", 2, 1, 1, 8, 8, 0.5, 1.0),
    ("odd", 3, 2, 65, 5, 7, 0.5, 1.0),
    ("big_grid", 4, 1, 1030, 128, 128, 2.0, 1.0),
    ("far", 5, 1, 64, 16, 16, 0.5, 3.0),
]
PERSP_CASE = "ragged"


def reference_available():
    return os.path.exists(os.path.join(REF, "utils", "projection.py"))


def load_reference():
    """The reference's utils/projection.py as a module of its own name space."""
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_reference_projection", os.path.join(REF, "utils", "projection.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cloud(seed, b, n, half):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, n, 3, generator=g) * (2 * half) - half


def generate(ref=None):
    ref = ref or load_reference()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the reference uses torch.range and an un-indexed meshgrid
        for name, seed, b, n, h, w, sigma_sq, half in CASES:
            xyz = cloud(seed, b, n, half)
            sil = ref.cont_proj(xyz, h, w, 'cpu', sigma_sq)
            assert sil.dtype == torch.float32 and tuple(sil.shape) == (b, h, w)
            out[f"{name}/xyz"] = xyz.numpy()
            out[f"{name}/sil"] = sil.numpy()
            print(f"{name}: B={b} N={n} {h}x{w} sigma_sq={sigma_sq} max={float(sil.max()):.4g} "
                  f"min={float(sil.min()):.4g}")
        src = torch.from_numpy(out[f"{PERSP_CASE}/xyz"]).clone()
        src[:, :, 2] += 2.5
        persp = ref.perspective_transform(src, 'cpu', src.shape[0])
        out["persp/xyz"] = src.numpy()
        out["persp/out"] = persp.contiguous().numpy()
    out["cases"] = np.array([c[0] for c in CASES])
    out["grids"] = np.array([[c[4], c[5]] for c in CASES], np.int32)
    out["sigma_sq"] = np.array([c[6] for c in CASES], np.float64)
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
