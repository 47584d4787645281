"""Host build of the REFERENCE's own Chamfer and EMD kernels (test infrastructure only).

The reference's native code is CUDA.  There is no nvcc here, but its two kernel
files need very little of CUDA: ``oracle/cuda_on_cpu/`` supplies that little
(``__global__``, ``__shared__``, ``threadIdx``, ``dim3``, the atomics, an
``at::Tensor`` stub, empty ``cuda.h`` / ``cuda_runtime.h``) and runs the threads
of a block as fibers that yield at ``__syncthreads()``.  The one construct that
is not C++, ``kernel<<<grid, block>>>(args)``, is rewritten by a regular
expression into ``CUDA_ON_CPU_LAUNCH(kernel, grid, block)(args)`` in a scratch
copy of each file.  g++ then compiles ``metric/emd/emd_cuda.cu`` and
``metric/chamfer3D/chamfer3D.cu`` otherwise unmodified into
``oracle/_ref/libpcm_ref_off.so``.

The library is the yardstick that ``pcm_oracle.c`` is pinned against
(tests/test_oracle_reference_cpu.py) and the source of the recorded outputs in
tests/golden/ref_kernels_golden.npz.  What it can and cannot pin:

  * STRUCTURE: tiling, tie order, the GetMax window, the double arithmetic of
    the bid value, NaN rules, the order of the backward's adds -- all of it is
    the reference's own text, executed.
  * NOT the floating-point contraction.  The build uses ``-ffp-contract=off``,
    so ``x*x+y*y+z*z`` is evaluated unfused; which FMA pattern nvcc picks for
    it cannot be observed without nvcc.  The oracle's ``order=1`` is the
    matching unfused evaluation; its default (``order=0``) is the fused
    pattern attributed to nvcc and stays unverified.
  * SCHEDULE: a GPU runs the threads of a grid in no defined order.  The
    emulator offers two, ascending and descending; racing plain stores (GetMax,
    emd_cuda.cu:188-191) are won by the last thread in that order.  Descending
    makes the LOWEST index win, which is the oracle's (and the product's)
    deterministic rule.  A case on which both schedules agree does not depend
    on the race at all.

Nothing from the reference is committed: the rewritten sources and the library
live in ``oracle/_ref/`` (git-ignored) and are rebuilt when stale.  Without the
reference directory ``build()`` returns None and ``available()`` is False.
The reference is found through ``PCM_REFERENCE`` (default as in
tests/golden/make_golden.py).
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SHIM = os.path.join(_HERE, "cuda_on_cpu")
OUT_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(OUT_DIR, "libpcm_ref_off.so")
SOURCES = (os.path.join("metric", "emd", "emd_cuda.cu"),
           os.path.join("metric", "chamfer3D", "chamfer3D.cu"))
CXXFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-fPIC", "-shared", "-w"]

_LAUNCH = re.compile(r"\b([A-Za-z_]\w*)\s*<<<(.*?)>>>\s*\(", re.S)
_lib = None


class ReferenceUnavailable(RuntimeError):
    pass


def reference_dir() -> str:
    return os.environ.get("PCM_REFERENCE", "/root/reference")


def _reference_sources():
    ref = reference_dir()
    paths = [os.path.join(ref, s) for s in SOURCES]
    return paths if all(os.path.isfile(p) for p in paths) else None


def _shim_files():
    return [os.path.join(_SHIM, f) for f in ("cuda_on_cpu.h", "cuda_on_cpu.cpp", "ref_entry.cpp")]


def rewrite_launches(text: str) -> str:
    """``k<<<cfg>>>(`` -> ``CUDA_ON_CPU_LAUNCH(k, cfg)(``; everything else untouched."""
    out, count = _LAUNCH.subn(lambda m: f"CUDA_ON_CPU_LAUNCH({m.group(1)}, {m.group(2)})(", text)
    if count == 0 or "<<<" in out:
        raise RuntimeError("kernel launches not rewritten as expected")
    return out


def build():
    """Compile oracle/_ref/libpcm_ref_off.so if missing or stale.

    Returns its path, or None ("unavailable") when the reference is absent."""
    srcs = _reference_sources()
    if srcs is None:
        return None
    deps = srcs + _shim_files() + [os.path.abspath(__file__)]
    if os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(d) for d in deps):
        return LIB_PATH
    os.makedirs(OUT_DIR, exist_ok=True)
    rewritten = []
    for src in srcs:
        dst = os.path.join(OUT_DIR, os.path.splitext(os.path.basename(src))[0] + ".cpp")
        with open(src, "r") as f:
            text = rewrite_launches(f.read())
        with open(dst, "w") as f:
            f.write(text)
        rewritten.append(dst)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    cmd = ([os.environ.get("CXX", "g++")] + CXXFLAGS
           + ["-I", _SHIM, "-I", os.path.join(_SHIM, "include"), "-include", "cuda_on_cpu.h", "-o", tmp]
           + rewritten + [os.path.join(_SHIM, "cuda_on_cpu.cpp"), os.path.join(_SHIM, "ref_entry.cpp")])
    subprocess.run(cmd, check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def available() -> bool:
    """True when the reference's kernels can be run here (builds them if need be)."""
    return build() is not None


def lib():
    global _lib
    if _lib is None:
        path = build()
        if path is None:
            raise ReferenceUnavailable(f"no reference kernels under {reference_dir()}")
        L = ctypes.CDLL(path)
        f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
        i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
        c_int, c_float = ctypes.c_int, ctypes.c_float
        L.cuda_on_cpu_set_descending.argtypes = [c_int]
        L.cuda_on_cpu_set_descending.restype = None
        L.pcm_ref_chamfer_forward.argtypes = [f32p, f32p, c_int, c_int, c_int, f32p, f32p, i32p, i32p]
        L.pcm_ref_chamfer_backward.argtypes = [f32p, f32p, c_int, c_int, c_int, f32p, f32p, f32p, f32p,
                                               i32p, i32p]
        L.pcm_ref_emd_forward.argtypes = [f32p, f32p, c_int, c_int, c_float, c_int, f32p, i32p, f32p,
                                          i32p, i32p, f32p, f32p, i32p, i32p, i32p, i32p, i32p]
        L.pcm_ref_emd_backward.argtypes = [f32p, f32p, c_int, c_int, f32p, f32p, i32p]
        for name in ("pcm_ref_chamfer_forward", "pcm_ref_chamfer_backward", "pcm_ref_emd_forward",
                     "pcm_ref_emd_backward"):
            getattr(L, name).restype = c_int
        _lib = L
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _checked(status, what):
    if status != 1:
        raise RuntimeError(f"reference {what} returned {status}")


def ref_emd_forward(xyz1, xyz2, eps: float, iters: int, descending: bool):
    """emd_cuda_forward under the chosen schedule -> (dist, assignment, price).

    State is initialised as the reference's wrapper does (emd_module.py:43-54):
    assignment = assignment_inv = -1, everything else zero."""
    xyz1, xyz2 = _f32(xyz1), _f32(xyz2)
    b, n, _ = xyz1.shape
    assert xyz2.shape == xyz1.shape and n % 1024 == 0 and b <= 512
    dist = np.zeros((b, n), np.float32)
    assignment = np.full((b, n), -1, np.int32)
    assignment_inv = np.full((b, n), -1, np.int32)
    price = np.zeros((b, n), np.float32)
    bid = np.zeros((b, n), np.int32)
    bid_increments = np.zeros((b, n), np.float32)
    max_increments = np.zeros((b, n), np.float32)
    unass_idx = np.zeros(b * n, np.int32)
    max_idx = np.zeros(b * n, np.int32)
    unass_cnt = np.zeros(512, np.int32)
    unass_cnt_sum = np.zeros(512, np.int32)
    cnt_tmp = np.zeros(512, np.int32)
    L = lib()
    L.cuda_on_cpu_set_descending(int(bool(descending)))
    _checked(L.pcm_ref_emd_forward(xyz1, xyz2, b, n, float(eps), int(iters), dist, assignment, price,
                                   assignment_inv, bid, bid_increments, max_increments, unass_idx,
                                   unass_cnt, unass_cnt_sum, cnt_tmp, max_idx), "emd_cuda_forward")
    return dist, assignment, price


def ref_emd_backward(xyz1, xyz2, graddist, assignment, descending: bool = False):
    """emd_cuda_backward into a zero-filled gradient (emd_module.py:83-86)."""
    xyz1, xyz2 = _f32(xyz1), _f32(xyz2)
    b, n, _ = xyz1.shape
    grad = np.zeros((b, n, 3), np.float32)
    L = lib()
    L.cuda_on_cpu_set_descending(int(bool(descending)))
    _checked(L.pcm_ref_emd_backward(xyz1, xyz2, b, n, grad, _f32(graddist), _i32(assignment)),
             "emd_cuda_backward")
    return grad


def ref_chamfer_forward(xyz1, xyz2, descending: bool = False):
    """chamfer_cuda_forward into zero-filled outputs (dist_chamfer_3D.py:40-52)
    -> dist1, dist2, idx1, idx2."""
    xyz1, xyz2 = _f32(xyz1), _f32(xyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    d1 = np.zeros((b, n), np.float32)
    d2 = np.zeros((b, m), np.float32)
    i1 = np.zeros((b, n), np.int32)
    i2 = np.zeros((b, m), np.int32)
    L = lib()
    L.cuda_on_cpu_set_descending(int(bool(descending)))
    _checked(L.pcm_ref_chamfer_forward(xyz1, xyz2, b, n, m, d1, d2, i1, i2), "chamfer_cuda_forward")
    return d1, d2, i1, i2


def ref_chamfer_backward(xyz1, xyz2, graddist1, graddist2, idx1, idx2, descending: bool = False):
    """chamfer_cuda_backward into zero-filled gradients (dist_chamfer_3D.py:63-68)."""
    xyz1, xyz2 = _f32(xyz1), _f32(xyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    g1 = np.zeros((b, n, 3), np.float32)
    g2 = np.zeros((b, m, 3), np.float32)
    L = lib()
    L.cuda_on_cpu_set_descending(int(bool(descending)))
    _checked(L.pcm_ref_chamfer_backward(xyz1, xyz2, b, n, m, g1, g2, _f32(graddist1), _f32(graddist2),
                                        _i32(idx1), _i32(idx2)), "chamfer_cuda_backward")
    return g1, g2


if __name__ == "__main__":
    print(build() or "unavailable")
