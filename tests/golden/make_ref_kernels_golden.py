#!/usr/bin/env python3
"""Record outputs of the REFERENCE's own Chamfer and EMD kernels for the GPU suite.

Runs only where the reference is present (it does not exist on the GPU
machines).  oracle/ref_build.py compiles the reference's chamfer3D.cu and
emd_cuda.cu for the host (-ffp-contract=off, threads as fibers); this script
runs them on a subset of tests/reference_cases.py and writes inputs and
outputs to tests/golden/ref_kernels_golden.npz, which
tests/test_reference_golden_gpu.py holds the HIP kernels to.

A case is recorded whole or REFUSED (no per-point exclusions):
  * the reference's assignment / argmins must equal the shipped oracle's
    (order=0, the FMA order the HIP kernels compute), so the recorded indices
    do not hinge on the one thing the host build cannot pin, the contraction;
  * a case labelled race-free must give the same bits under the ascending and
    the descending schedule.  The others are recorded under the descending
    schedule (lowest index wins GetMax, the product's deterministic rule).

Indices are stored as int16 (every cloud here has <= 4096 points).

Usage:  python tests/golden/make_ref_kernels_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import oracle as O  # noqa: E402
import ref_build  # noqa: E402
import reference_cases as C  # noqa: E402

OUT = os.path.join(HERE, "ref_kernels_golden.npz")
EMD_RECORDED = ("b2_n1024_eps005", "converged_n1024", "exact_ties_n4096",
                "scale_1e-4", "scale_1e3", "small_scale_big_eps")
EMD_BACKWARD = "b2_n1024_eps005"
CHAMFER_RECORDED = ("nan_tiles_700x1300", "nan_tile3_300x1600", "finite_500x900")
CHAMFER_BACKWARD = "finite_500x900"
MAX_POINTS = 4096


def refuse(name, why):
    raise SystemExit(f"REFUSED {name}: {why}")


def same_bits(x, y):
    return np.array_equal(x.view(np.int32), y.view(np.int32))


def main():
    if not ref_build.available():
        raise SystemExit(f"no reference kernels under {ref_build.reference_dir()}")
    O.build()
    out = {}
    for name in EMD_RECORDED:
        make, eps, iters, race_free, _ = C.EMD_CASES[name]
        a, c = make()
        if a.shape[1] > MAX_POINTS:
            refuse(name, "cloud larger than the fixture allows")
        dist, ass, price = ref_build.ref_emd_forward(a, c, eps, iters, descending=True)
        if race_free:
            for x, y in zip((dist, ass, price), ref_build.ref_emd_forward(a, c, eps, iters, descending=False)):
                if not same_bits(x, y):
                    refuse(name, "labelled race-free but the schedules disagree")
        _, oracle_ass = O.emd_forward(a, c, eps, iters)
        if not np.array_equal(ass, oracle_ass):
            refuse(name, "reference assignment differs from the shipped oracle's")
        out[f"emd/{name}/xyz1"] = a
        out[f"emd/{name}/xyz2"] = c
        out[f"emd/{name}/eps"] = np.float32(eps)
        out[f"emd/{name}/iters"] = np.int32(iters)
        out[f"emd/{name}/dist"] = dist
        out[f"emd/{name}/assignment"] = ass.astype(np.int16)
        if name == EMD_BACKWARD:
            gd = C.graddist(300, *dist.shape)
            out[f"emd/{name}/graddist"] = gd
            out[f"emd/{name}/gradxyz1"] = ref_build.ref_emd_backward(a, c, gd, ass)
        print(f"emd {name}: B={a.shape[0]} N={a.shape[1]} eps={eps} iters={iters} recorded")
    for name in CHAMFER_RECORDED:
        a, c = C.CHAMFER_FORWARD_CASES[name]()
        d1, d2, i1, i2 = ref_build.ref_chamfer_forward(a, c)
        for x, y in zip((d1, d2, i1, i2), ref_build.ref_chamfer_forward(a, c, descending=True)):
            if not same_bits(x, y):
                refuse(name, "the schedules disagree")
        _, _, j1, j2 = O.chamfer_forward(a, c)
        if not (np.array_equal(i1, j1) and np.array_equal(i2, j2)):
            refuse(name, "reference argmins differ from the shipped oracle's")
        out[f"chamfer/{name}/xyz1"] = a
        out[f"chamfer/{name}/xyz2"] = c
        out[f"chamfer/{name}/dist1"] = d1
        out[f"chamfer/{name}/dist2"] = d2
        out[f"chamfer/{name}/idx1"] = i1.astype(np.int16)
        out[f"chamfer/{name}/idx2"] = i2.astype(np.int16)
        if name == CHAMFER_BACKWARD:
            gd1, gd2 = C.graddist(301, *d1.shape), C.graddist(302, *d2.shape)
            g1, g2 = ref_build.ref_chamfer_backward(a, c, gd1, gd2, i1, i2)  # ascending schedule
            out[f"chamfer/{name}/graddist1"] = gd1
            out[f"chamfer/{name}/graddist2"] = gd2
            out[f"chamfer/{name}/gradxyz1"] = g1
            out[f"chamfer/{name}/gradxyz2"] = g2
        print(f"chamfer {name}: B={a.shape[0]} N={a.shape[1]} M={c.shape[1]} recorded")
    out["emd_cases"] = np.array(EMD_RECORDED)
    out["chamfer_cases"] = np.array(CHAMFER_RECORDED)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
