"""Chamfer distance of D-dimensional clouds, 1 <= D <= 8 (pcm_chamfer_nd_forward /
pcm_chamfer_nd_backward, csrc/chamfer_nd.hip; the contract is in include/pcm.h).

``chamfer_NDFunction`` / ``chamfer_NDDist()(input1, input2) -> (dist1, dist2,
idx1, idx2)`` take float32 device clouds [B, N, D] and [B, M, D]; distances are
float32, indices int32 and non-differentiable, as chamfer_3DDist's.  The thin
subclasses ``chamfer_2DDist``, ``chamfer_5DDist`` and ``chamfer_6DDist`` (with
``chamfer_2DFunction`` ...) carry the names of upstream ChamferDistancePytorch's
chamfer2D / chamfer5D / chamfer6D modules and assert their dimension with
upstream's message (INTEGRATION.md maps the imports).

As in dist_chamfer_3D.py: outputs are allocated on the device and zero-filled
only when a cloud is empty; a [B, N, D] view of a contiguous [B, D, N] tensor
(a network output passed as .transpose(2, 1)) is read in place and its
gradient written in the same layout; anything else is made contiguous; a
None graddist (an unused output) counts as zeros; CPU tensors, other dtypes, a
D outside 1..8 or two different D raise.  A D = 3 call runs the N-D kernels,
not chamfer_3DDist's: the two differ on NaN distances (include/pcm.h).
"""
import os
import sys

import torch
from torch import nn
from torch.autograd import Function

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcm_hip  # noqa: E402

_WRONG_DIM = "Wrong last dimension for the chamfer distance 's input! Check with .size()"


def _in_place(t):
    """(tensor, layout): t itself where the kernels read it in place, else a contiguous copy."""
    lay = pcm_hip.cloud_layout_nd(t)
    if lay is None:
        return t.contiguous(), 0
    return t, lay


def _empty_like_layout(t, lay):
    b, n, d = t.shape
    if lay == 1:
        return torch.empty(b, d, n, dtype=t.dtype, device=t.device).transpose(1, 2)
    return torch.empty(b, n, d, dtype=t.dtype, device=t.device)


def _graddist(g, idx):
    if g is None:  # an unused output
        return torch.zeros(idx.shape, dtype=torch.float32, device=idx.device)
    return g.contiguous().float()


class chamfer_NDFunction(Function):
    DIM = None  # a subclass fixes its dimension

    @classmethod
    def _check(cls, xyz1, xyz2):
        if xyz1.dim() != 3 or xyz2.dim() != 3:
            raise ValueError("the chamfer distance takes clouds [B, N, D] and [B, M, D]")
        d1, d2 = xyz1.size(2), xyz2.size(2)
        if cls.DIM is not None:
            assert d1 == cls.DIM, _WRONG_DIM
            assert d2 == cls.DIM, _WRONG_DIM
        if d1 != d2:
            raise ValueError(f"the clouds have {d1} and {d2} coordinates a point")
        if not 1 <= d1 <= pcm_hip.CHAMFER_ND_MAX_DIM:
            raise ValueError(f"chamfer_NDFunction takes 1..{pcm_hip.CHAMFER_ND_MAX_DIM} coordinates a point (got {d1})")
        assert xyz2.size(0) == xyz1.size(0), "batch sizes of the two clouds differ"
        if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
            raise TypeError("chamfer_NDFunction expects float32 clouds")
        if not (xyz1.is_cuda and xyz2.is_cuda):
            raise RuntimeError("chamfer_NDFunction needs HIP device tensors; there is no CPU path")

    @classmethod
    def forward(cls, ctx, xyz1, xyz2):
        cls._check(xyz1, xyz2)
        xyz1, lay1 = _in_place(xyz1)
        xyz2, lay2 = _in_place(xyz2)
        batchsize, n, _ = xyz1.size()
        m = xyz2.size(1)
        device = xyz1.device
        # the kernel writes every output element unless a cloud is empty, where the outputs are zeros
        alloc = torch.zeros if (n == 0 or m == 0) else torch.empty
        dist1 = alloc(batchsize, n, device=device)
        dist2 = alloc(batchsize, m, device=device)
        idx1 = alloc(batchsize, n, dtype=torch.int32, device=device)
        idx2 = alloc(batchsize, m, dtype=torch.int32, device=device)
        pcm_hip.chamfer_nd_forward(xyz1, lay1, xyz2, lay2, dist1, dist2, idx1, idx2)
        ctx.layouts = (lay1, lay2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        ctx.set_materialize_grads(False)  # no fill kernels for the unused outputs' gradients
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        lay1, lay2 = ctx.layouts
        grad1, grad2 = _empty_like_layout(xyz1, lay1), _empty_like_layout(xyz2, lay2)
        pcm_hip.chamfer_nd_backward(xyz1, lay1, xyz2, lay2, _graddist(graddist1, idx1), _graddist(graddist2, idx2),
                                    idx1, idx2, grad1, grad2)
        return grad1, grad2


class chamfer_NDDist(nn.Module):
    function = chamfer_NDFunction

    def forward(self, input1, input2):
        return self.function.apply(input1, input2)


class chamfer_2DFunction(chamfer_NDFunction):
    DIM = 2


class chamfer_5DFunction(chamfer_NDFunction):
    DIM = 5


class chamfer_6DFunction(chamfer_NDFunction):
    DIM = 6


class chamfer_2DDist(chamfer_NDDist):
    function = chamfer_2DFunction


class chamfer_5DDist(chamfer_NDDist):
    function = chamfer_5DFunction


class chamfer_6DDist(chamfer_NDDist):
    function = chamfer_6DFunction
