"""Repulsion loss -- PU-GAN's point-distribution regulariser, the
``get_repulsion_loss`` the reference's loss class once had (the ``repulsion_loss``
column of test_pix.py:26,72 is what is left of it), as ONE pcm_repulsion_loss
call behind an autograd Function (csrc/knn.hip; include/pcm.h has the
contract): the k = 5 self search, the loss and its full gradient.

The reference's version searched with knn_cuda under ``torch.no_grad()`` and
formed the loss from the returned distances, so it carried no gradient at all.
This one is differentiable: every active term pushes both of its points apart.
"""
import os
import sys

import torch
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


class repulsion_lossFunction(Function):
    """mean over points and their list slots 1..4 of max(0, h - squared
    distance), float32 [B, N, 3] clouds (rows, or a view of channel planes,
    read in place); differentiable in the cloud.  Loss and gradient come from
    the one call in ``forward``; the gradient has the cloud's layout.  An empty
    batch (B = 0) gives NaN, the mean over nothing as ``torch.mean`` has it, and
    an empty gradient: the library call is a no-op there."""

    @staticmethod
    def forward(ctx, xyz, h):
        if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32:
            raise TypeError("the repulsion loss expects a float32 cloud")
        if xyz.dim() != 3 or xyz.size(2) != 3:
            raise ValueError("the repulsion loss expects a cloud [B, N, 3]")
        if xyz.size(1) < pcm_hip.REPULSION_K:
            raise ValueError(f"the repulsion loss needs clouds of at least {pcm_hip.REPULSION_K} points")
        if not xyz.is_cuda:
            raise RuntimeError(f"the repulsion loss needs a HIP device tensor (got one on {xyz.device}); "
                               "there is no CPU path")
        pts = xyz.detach()
        lay = pcm_hip.cloud_layout(pts)
        if lay is None:
            pts, lay = pts.contiguous(), 0
        loss = torch.empty((), dtype=torch.float32, device=pts.device)
        if pts.size(0) == 0:
            loss.fill_(float("nan"))  # the mean over nothing, as torch.mean's
        grad = None
        if ctx.needs_input_grad[0]:
            # empty_like keeps a planes view's strides: the gradient is written in the cloud's layout
            grad = torch.empty_like(pts) if lay == 0 else torch.empty_like(pts.transpose(1, 2)).transpose(1, 2)
        pcm_hip.repulsion_loss(pts, lay, float(h), loss.view(1), grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return grad_loss * grad, None
