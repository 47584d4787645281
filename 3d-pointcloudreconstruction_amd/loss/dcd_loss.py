"""Density-aware Chamfer distance (Wu et al., "Density-aware Chamfer Distance
as a Comprehensive Metric for Point Cloud Completion", NeurIPS 2021):

    DCD(x, gt) = 1/2 ( mean_q [1 - exp(-alpha d(q)) r / (c(nn(q))^lambda + 1e-6)]  over gt's points
                     + the same over x's points ),

d the squared distance of a point to its nearest neighbour nn(q) in the other
cloud, c how many points share that neighbour and r = |queries| / |targets|.
Chamfer lets many predicted points share one ground-truth neighbour at no cost;
DCD divides every term by that count and bounds it by 1.  The formula is stated
from the published source, not verified against it (the package is not
installed where this was written); include/pcm.h has the contract.

The whole batch is ONE pcm_dcd_loss call behind an autograd Function
(csrc/dcd.hip): the Chamfer forward, one launch for both hit-count histograms,
the terms, the per-point upstream weights and the sums, and the Chamfer
backward when a cloud needs a gradient.  The published code runs the step
between forward and backward as a Python loop over the batch (bincount, gather,
pow, reciprocal, multiply, mean, stack); this call has no loop, no host
synchronisation and no allocation of its own, so it is capturable in a graph.

``alpha = 1000`` is the published default and suits clouds of about 2048
points or more in a unit box.  At 1024 uniform points it already gives a loss
of 0.91, and below a few hundred points every term is 1 to float32: coarse
outputs of 128 or 256 points need a smaller alpha (about 1 / the median squared
nearest-neighbour distance keeps exp(-alpha d) near 0.4).

Difference from the published ``calc_dcd``: ``cd_p`` and ``cd_t`` come
detached; training on the Chamfer distance is ``chamfer_3DDist``'s job.
"""
import math
import os
import sys

import torch
from torch import nn
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


def _like(pts, lay):
    """An uninitialised tensor of the cloud's shape and layout."""
    return torch.empty_like(pts) if lay == 0 else torch.empty_like(pts.transpose(1, 2)).transpose(1, 2)


def _checked(alpha, n_lambda):
    alpha, n_lambda = float(alpha), float(n_lambda)
    if not (math.isfinite(alpha) and alpha > 0):
        raise ValueError(f"the DCD loss needs a finite alpha > 0 (got {alpha})")
    if not (math.isfinite(n_lambda) and n_lambda >= 0):
        raise ValueError(f"the DCD loss needs a finite n_lambda >= 0 (got {n_lambda})")
    return alpha, n_lambda


def _clouds(x, gt):
    """[(points, layout)] of both clouds, detached, read in place where the layout allows."""
    for t in (x, gt):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("the DCD loss expects float32 clouds")
        if t.dim() != 3 or t.size(2) != 3:
            raise ValueError("the DCD loss expects clouds [B, N, 3] and [B, M, 3]")
    if x.size(0) != gt.size(0):
        raise ValueError("the DCD loss expects clouds of one batch size")
    if not (x.is_cuda and gt.is_cuda):
        raise RuntimeError(f"the DCD loss needs HIP device tensors (got {x.device} and {gt.device}); "
                           "there is no CPU path")
    out = []
    for t in (x, gt):
        pts = t.detach()
        lay = pcm_hip.cloud_layout(pts)
        if lay is None:
            pts, lay = pts.contiguous(), 0
        out.append((pts, lay))
    return out


class dcd_lossFunction(Function):
    """``apply(x, gt, alpha, n_lambda, non_reg, workspace)``: the [B] density-aware Chamfer
    distances of the float32 clouds x [B, N, 3] and gt [B, M, 3] (rows, or views
    of channel planes, read in place), and [B, 2] holding cd_p and cd_t (not
    differentiable).  The unit gradients come from the one call in ``forward``
    -- only those ``ctx.needs_input_grad`` asks for, in their cloud's layout --
    and ``backward`` scales them by the upstream [B] gradient.  ``workspace``
    (optional): a uint8 device tensor of ``pcm_hip.dcd_workspace_bytes(B, N, M)``
    bytes, else the cached buffer of the current stream."""

    @staticmethod
    def forward(ctx, x, gt, alpha=1000.0, n_lambda=1.0, non_reg=False, workspace=None):
        alpha, n_lambda = _checked(alpha, n_lambda)
        (p1, l1), (p2, l2) = _clouds(x, gt)
        if (l1 or l2) and pcm_hip.load_library().pcm_chamfer_forward_ws_bytes(p1.size(0), p1.size(1), p2.size(1)) > 0:
            # the grid forward of large clouds reads rows, and pays for the copy
            (p1, l1), (p2, l2) = (p1.contiguous(), 0), (p2.contiguous(), 0)
        loss = torch.empty(p1.size(0), dtype=torch.float32, device=p1.device)
        cd = torch.empty(p1.size(0), 2, dtype=torch.float32, device=p1.device)
        g1 = _like(p1, l1) if ctx.needs_input_grad[0] else None
        g2 = _like(p2, l2) if ctx.needs_input_grad[1] else None
        pcm_hip.dcd_loss(p1, l1, p2, l2, alpha, n_lambda, non_reg, loss, cd, g1, g2, workspace=workspace)
        ctx.save_for_backward(g1, g2)
        ctx.mark_non_differentiable(cd)
        return loss, cd

    @staticmethod
    def backward(ctx, grad_loss, _grad_cd):
        g1, g2 = ctx.saved_tensors
        w = grad_loss.reshape(-1, 1, 1)
        return (None if g1 is None else w * g1), (None if g2 is None else w * g2), None, None, None, None


def calc_dcd(x, gt, alpha=1000, n_lambda=1, return_raw=False, non_reg=False, workspace=None):
    """The published ``calc_dcd``: ``[loss, cd_p, cd_t]``, each [B]; ``loss`` is
    differentiable in both clouds, ``cd_p`` and ``cd_t`` are detached.  With
    ``return_raw`` also ``dist1, dist2, idx1, idx2`` in the published
    convention: ``dist1`` [B, M] and ``idx1`` belong to gt's points (each gt
    point's nearest neighbour in x), ``dist2`` [B, N] and ``idx2`` to x's.  They
    come from one more Chamfer forward, outside autograd.  ``workspace``: see
    ``dcd_lossFunction`` (an addition to the published signature)."""
    loss, cd = dcd_lossFunction.apply(x, gt, alpha, n_lambda, non_reg, workspace)
    res = [loss, cd[:, 0], cd[:, 1]]
    if return_raw:
        (p1, l1), (p2, l2) = _clouds(x, gt)
        b, n, m = p1.size(0), p1.size(1), p2.size(1)
        d_x = torch.empty(b, n, dtype=torch.float32, device=p1.device)
        d_gt = torch.empty(b, m, dtype=torch.float32, device=p1.device)
        i_x = torch.empty(b, n, dtype=torch.int32, device=p1.device)
        i_gt = torch.empty(b, m, dtype=torch.int32, device=p1.device)
        if l1 == 0 and l2 == 0:
            pcm_hip.chamfer_forward(p1, p2, d_x, d_gt, i_x, i_gt)
        else:
            pcm_hip.chamfer_forward_layout(p1, p2, l1, l2, d_x, d_gt, i_x, i_gt)
        res.extend([d_gt, d_x, i_gt, i_x])
    return res


class DCDLoss(nn.Module):
    """``DCDLoss(alpha, n_lambda, non_reg)(x, gt)``: the batch mean of the
    density-aware Chamfer distance of x [B, N, 3] and gt [B, M, 3]."""

    def __init__(self, alpha=1000, n_lambda=1, non_reg=False):
        super().__init__()
        self.alpha, self.n_lambda = _checked(alpha, n_lambda)
        self.non_reg = bool(non_reg)

    def forward(self, x, gt):
        loss, _ = dcd_lossFunction.apply(x, gt, self.alpha, self.n_lambda, self.non_reg)
        return torch.mean(loss)
