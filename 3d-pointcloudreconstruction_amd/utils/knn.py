"""k nearest neighbours -- the ``knn_cuda.KNN`` the reference's loss class was
written around: loss/loss.py:16-17 still carries the commented-out
``KNN(k=2, transpose_mode=True)`` and ``KNN(k=20, transpose_mode=True)``
members, and its dropped ``get_repulsion_loss`` / ``get_uniform_loss`` called
them as ``knn(ref, query)``.

``knn_cuda`` is not installed here, so the interface is taken from those call
sites: ``KNN(k, transpose_mode)(ref, query)`` returns ``(dist, idx)``, the
Euclidean distances and the int64 indices into ``ref`` of every query's k
nearest reference points, nearest first.

Both go through one launch of pcm_knn (csrc/knn.hip; include/pcm.h has the
contract): every query's list stays in registers, ties go to the lower index,
and slots without a candidate hold (+inf, -1).

Differences:
  * clouds are 3-D float32 with at most pcm_hip.KNN_MAX_POINTS points and
    k <= pcm_hip.KNN_MAX_K, on a HIP device: all compute goes through
    libpcm_hip.so and CPU tensors raise;
  * a [B, N, 3] view of contiguous [B, 3, N] planes is read in place
    (pcm_hip.cloud_layout), so ``transpose_mode=False`` copies nothing; other
    strides are made contiguous first;
  * ``knn_points`` returns the SQUARED distances in the library's pinned order
    fma(dz, dz, fma(dy, dy, dx * dx)) and int32 indices, exactly as the kernel
    wrote them; ``KNN`` takes their square root and widens the indices;
  * outputs are not differentiable (knn_cuda's ran under torch.no_grad());
    loss/repulsion_loss.py is the differentiable caller.
"""
import os
import sys

import torch
import torch.nn as nn

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


def _check(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"k nearest neighbours expects float32 clouds ({name})")
    if t.dim() != 3 or t.size(2) != 3:
        raise ValueError(f"k nearest neighbours expects clouds [B, N, 3] ({name})")


def _cloud(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"k nearest neighbours needs HIP device tensors (got {name} on {t.device}); "
                           "there is no CPU path")
    t = t.detach()
    lay = pcm_hip.cloud_layout(t)
    if lay is None:
        t, lay = t.contiguous(), 0
    return t, lay


def knn_points(query, ref, k):
    """(dist, idx) of one pcm_knn launch: for every point of ``query`` [B, N, 3]
    its ``k`` nearest points of ``ref`` [B, M, 3] -- dist [B, N, k] float32
    SQUARED distances, ascending, and idx [B, N, k] int32 into ``ref``; equal
    distances go to the lower index; slots without a candidate (M < k,
    non-finite points) hold (+inf, -1).  Detached: no gradient flows."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    _check(query, "query")
    _check(ref, "ref")
    query, lay_q = _cloud(query, "query")
    ref, lay_r = _cloud(ref, "ref")
    if ref.size(0) != query.size(0):
        raise ValueError("query and ref differ in batch size")
    b, n = query.size(0), query.size(1)
    dist = torch.empty(b, n, k, dtype=torch.float32, device=query.device)
    idx = torch.empty(b, n, k, dtype=torch.int32, device=query.device)
    pcm_hip.knn(query, lay_q, ref, lay_r, k, dist, idx)
    return dist, idx


class KNN(nn.Module):
    """``KNN(k, transpose_mode)(ref, query)`` -> (dist, idx), the calling
    convention of knn_cuda at the reference's call sites.
    ``transpose_mode=True``: ref [B, M, 3], query [B, N, 3], outputs [B, N, k];
    ``transpose_mode=False``: ref [B, 3, M], query [B, 3, N], outputs [B, k, N].
    dist is Euclidean (float32), idx int64; neither is differentiable."""

    def __init__(self, k, transpose_mode=False):
        super(KNN, self).__init__()
        self.k = int(k)
        self.transpose_mode = bool(transpose_mode)

    def forward(self, ref, query):
        if not self.transpose_mode:
            for t in (ref, query):
                if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.size(1) != 3:
                    raise ValueError("KNN(transpose_mode=False) expects clouds [B, 3, N]")
            ref, query = ref.transpose(1, 2), query.transpose(1, 2)
        dist, idx = knn_points(query, ref, self.k)
        dist, idx = torch.sqrt(dist), idx.long()
        if not self.transpose_mode:
            dist, idx = dist.transpose(1, 2).contiguous(), idx.transpose(1, 2).contiguous()
        return dist, idx
