"""Debiased Sinkhorn divergence between two point clouds -- what geomloss's
``SamplesLoss(loss='sinkhorn', p=2)`` computes for unweighted clouds, and what
the reference's ``batch_EMD_loss`` (loss/loss_.py:111-120) is named after.  The
whole batch is ONE pcm_sinkhorn_loss call behind an autograd Function
(csrc/sinkhorn.hip; include/pcm.h has the contract):

    S(x, y) = OT_eps(x, y) - 1/2 OT_eps(x, x) - 1/2 OT_eps(y, y),  eps = blur^2,
    cost |x - y|^2 / 2, weights 1/N and 1/M,

reached by the symmetric Sinkhorn loop with averaged updates and
epsilon-scaling from diameter^2 down to blur^2 by a factor scaling^2 a step,
and a last extrapolation step that also gives the gradients.  It is defined
for any N and M (N != M included), differentiable in both clouds, and
interpolates between the energy-type kernel norm (large blur) and the earth
mover's distance (small blur): the transport loss for the generator's 128- and
256-point coarse outputs, which the auction EMD (N = M = a multiple of 1024, no
gradient for the second cloud) cannot take.

geomloss is not installed where this module was written and could not be
fetched: the algorithm is its published one (sinkhorn_loop) and is not verified
against the package.

``SamplesLoss`` here also takes the kernel-norm names and hands them to
loss/kernel_loss.py.
"""
import os
import sys

import torch
from torch import nn
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.append(_HERE)
import pcm_hip  # noqa: E402
import kernel_loss  # noqa: E402


def _like(pts, lay):
    """An uninitialised tensor of the cloud's shape and layout."""
    return torch.empty_like(pts) if lay == 0 else torch.empty_like(pts.transpose(1, 2)).transpose(1, 2)


def joint_diameter(x, y):
    """The larger extent of the joint bounding box of x [B, N, 3] and y
    [B, M, 3] over the whole batch, as a Python float: ONE host read-back.  A
    batch of coincident points gives 1.0 (any positive value serves there)."""
    lo = torch.minimum(x.detach().amin(dim=(0, 1)), y.detach().amin(dim=(0, 1)))
    hi = torch.maximum(x.detach().amax(dim=(0, 1)), y.detach().amax(dim=(0, 1)))
    d = float((hi - lo).max().item())
    return d if d > 0 else 1.0


class sinkhorn_lossFunction(Function):
    """``apply(x, y, blur, scaling, diameter)``: the [B] Sinkhorn divergences
    of the float32 clouds x [B, N, 3] and y [B, M, 3] (rows, or views of
    channel planes, read in place); ``diameter`` is a host number.  The unit
    gradients come from the one call in ``forward`` -- only those
    ``ctx.needs_input_grad`` asks for, in their cloud's layout -- and
    ``backward`` scales them by the upstream [B] gradient."""

    @staticmethod
    def forward(ctx, x, y, blur, scaling, diameter):
        for t in (x, y):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("the Sinkhorn loss expects float32 clouds")
            if t.dim() != 3 or t.size(2) != 3:
                raise ValueError("the Sinkhorn loss expects clouds [B, N, 3] and [B, M, 3]")
        if x.size(0) != y.size(0):
            raise ValueError("the Sinkhorn loss expects clouds of one batch size")
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError(f"the Sinkhorn loss needs HIP device tensors (got {x.device} and {y.device}); "
                               "there is no CPU path")
        clouds = []
        for t in (x, y):
            pts = t.detach()
            lay = pcm_hip.cloud_layout(pts)
            if lay is None:
                pts, lay = pts.contiguous(), 0
            clouds.append((pts, lay))
        (p1, l1), (p2, l2) = clouds
        loss = torch.empty(p1.size(0), dtype=torch.float32, device=p1.device)
        g1 = _like(p1, l1) if ctx.needs_input_grad[0] else None
        g2 = _like(p2, l2) if ctx.needs_input_grad[1] else None
        pcm_hip.sinkhorn_loss(p1, l1, p2, l2, float(blur), float(scaling), float(diameter), loss, g1, g2)
        ctx.save_for_backward(g1, g2)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g1, g2 = ctx.saved_tensors
        w = grad_loss.reshape(-1, 1, 1)
        return (None if g1 is None else w * g1), (None if g2 is None else w * g2), None, None, None


class SamplesLoss(nn.Module):
    """geomloss's calling convention for unweighted clouds: ``SamplesLoss(loss,
    p, blur, scaling, diameter)(x, y)`` with x [N, 3] and y [M, 3] gives a
    scalar, with x [B, N, 3] and y [B, M, 3] one value per batch element.

    ``loss='sinkhorn'``: the debiased divergence at ``blur`` with
    epsilon-scaling ratio ``scaling`` in (0, 1).  ``diameter=None`` takes the
    larger extent of the clouds' joint bounding box over the batch with torch,
    which reads one number back to the host on every call; passing a diameter
    (an upper bound of the extent: sqrt(3) covers the unit cube) keeps the call
    free of host synchronisation and capturable in a graph.  ``loss`` in
    'gaussian', 'laplacian', 'energy' delegates to kernel_loss.SamplesLoss.
    ``p != 2``, ``debias=False``, ``reach`` and weighted calls raise
    NotImplementedError."""

    def __init__(self, loss="sinkhorn", p=2, blur=0.05, scaling=0.5, diameter=None, debias=True, reach=None,
                 **kwargs):
        super().__init__()
        self.kernel = None
        if loss in kernel_loss.KERNELS:
            if reach is not None:
                kwargs["reach"] = reach
            self.kernel = kernel_loss.SamplesLoss(loss, p=p, blur=blur, **kwargs)
        elif loss != "sinkhorn":
            raise NotImplementedError(f"SamplesLoss(loss={loss!r}) is not offered here: 'sinkhorn' and the kernel "
                                      f"norms {sorted(kernel_loss.KERNELS)} are")
        else:
            if p != 2:
                raise NotImplementedError(f"SamplesLoss('sinkhorn', p={p!r}) is not offered here: p = 2 is")
            if not debias:
                raise NotImplementedError("SamplesLoss('sinkhorn', debias=False) is not offered here")
            if reach is not None:
                raise NotImplementedError("SamplesLoss('sinkhorn', reach=...) (unbalanced transport) is not "
                                          "offered here")
            if kwargs:
                raise NotImplementedError(f"SamplesLoss options {sorted(kwargs)} are not offered here")
            if not float(blur) > 0:
                raise ValueError("blur must be positive")
            if not 0 < float(scaling) < 1:
                raise ValueError("scaling must lie in (0, 1)")
            if diameter is not None and not float(diameter) > 0:
                raise ValueError("diameter must be positive")
        self.loss, self.p, self.blur, self.scaling = loss, p, float(blur), float(scaling)
        self.diameter = None if diameter is None else float(diameter)

    def forward(self, *args):
        if self.kernel is not None:
            return self.kernel(*args)
        if len(args) != 2:
            raise NotImplementedError("weighted clouds (alpha, x, beta, y) are not offered here: SamplesLoss "
                                      "takes (x, y) with uniform weights")
        x, y = args
        single = x.dim() == 2 and y.dim() == 2
        if single:
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        diameter = self.diameter
        if (diameter is None and x.is_cuda and y.is_cuda and x.dim() == 3 and y.dim() == 3
                and x.size(2) == 3 == y.size(2) and x.numel() and y.numel()):
            diameter = joint_diameter(x, y)
        out = sinkhorn_lossFunction.apply(x, y, self.blur, self.scaling, 1.0 if diameter is None else diameter)
        return out[0] if single else out
