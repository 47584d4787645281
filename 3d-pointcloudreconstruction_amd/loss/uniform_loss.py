"""Uniform loss -- PU-GAN's other point-distribution regulariser, the
``get_uniform_loss`` the reference's loss class once had (the ``uniform_loss``
column of test_pix.py:26,72 is what is left of its caller), as ONE
pcm_uniform_loss call behind an autograd Function (csrc/grouping.hip;
include/pcm.h has the contract): farthest point seeds, a ball query per scale
around every seed, each group member's nearest other member, the loss and its
full gradient.

The reference's version composed pointnet2_ops' sampling and grouping with a
knn_cuda search of every group against itself; both ran outside autograd, so
its loss carried no gradient.  This one is differentiable in the cloud (seeds,
ball membership and the choice of neighbour carry none), and a slot whose
nearest other member is at distance zero -- a padding copy, coincident points
-- contributes nothing, where the square root's derivative would be infinite.
The ball query's padding rule is pointnet2's published one, not verified
against pointnet2_ops (utils/pointnet2_utils.py).
"""
import os
import sys

import torch
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


class uniform_lossFunction(Function):
    """``apply(xyz, npoint, nsample, ball_radius, weight, expect_len)``: the
    sum over the scales q of weight[q] times the mean, over the ``npoint``
    farthest point seeds of every cloud, of (m - expect_len)^2 / (expect_len +
    1e-8), m the mean distance of a group member to its nearest other member in
    the seed's ball of radius ball_radius[q], cut to its first nsample[q]
    points.  float32 [B, N, 3] clouds (rows, or a view of channel planes, read
    in place).  Loss and gradient come from the one call in ``forward``; the
    gradient has the cloud's layout.  An empty batch (B = 0) gives NaN, the mean
    over nothing as ``torch.mean`` has it, and an empty gradient."""

    @staticmethod
    def forward(ctx, xyz, npoint, nsample, ball_radius, weight, expect_len):
        if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32:
            raise TypeError("the uniform loss expects a float32 cloud")
        if xyz.dim() != 3 or xyz.size(2) != 3:
            raise ValueError("the uniform loss expects a cloud [B, N, 3]")
        nsample = [int(v) for v in nsample]
        if int(npoint) < 1:
            raise ValueError("the uniform loss needs at least one seed")
        if not 1 <= len(nsample) <= pcm_hip.UNIFORM_MAX_SCALES:
            raise ValueError(f"the uniform loss takes 1 to {pcm_hip.UNIFORM_MAX_SCALES} scales")
        if min(nsample) < 2 or max(nsample) > pcm_hip.BALL_MAX_NSAMPLE:
            raise ValueError(f"the uniform loss takes groups of 2 to {pcm_hip.BALL_MAX_NSAMPLE} points")
        if not xyz.is_cuda:
            raise RuntimeError(f"the uniform loss needs a HIP device tensor (got one on {xyz.device}); "
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
        pcm_hip.uniform_loss(pts, lay, int(npoint), nsample, ball_radius, weight, float(expect_len), loss.view(1),
                             grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return grad_loss * grad, None, None, None, None, None
