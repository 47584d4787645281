"""Kernel-norm (MMD) losses between two point clouds -- the working counterpart
of the reference's ``batch_EMD_loss`` (loss/loss_.py:111-120), which calls
geomloss's ``SamplesLoss(loss='gaussian', p=2, blur=.00005)`` once per cloud
in a Python loop.  Here the whole batch is ONE pcm_kernel_loss call behind an
autograd Function (csrc/kernel_loss.hip; include/pcm.h has the contract):

    L = 1/2 sum a a k(x_i, x_i') + 1/2 sum b b k(y_j, y_j') - sum a b k(x_i, y_j),
    a = 1/N, b = 1/M,  sigma = blur,
    k = exp(-|x-y|^2 / (2 sigma^2))   'gaussian'
    k = exp(-|x-y| / sigma)           'laplacian'
    k = -|x-y|                        'energy' (blur is not used)

differentiable in both clouds, defined for any N and M (N != M included), with
no assignment or argmin in it.  ``loss='gaussian'`` is not a Sinkhorn
divergence and, despite the reference's name for it, not an earth mover's
distance; ``loss='sinkhorn'`` is not offered by this module: loss/sinkhorn_loss.py has
it (and delegates the kernel norms here).

geomloss is not installed where this module was written and could not be
fetched: the formulas are its published ones and are not verified against the
package.  One known deviation: geomloss's dense path clamps the squared
distance at 1e-8 before the square root; here a coincident pair has distance
zero exactly and adds nothing to a Laplacian or energy gradient (the
subgradient).

A note on the reference's blur.  At blur = 5e-5 every off-diagonal term
exp(-d^2 / 5e-9) underflows for ordinary clouds (two points 1e-3 apart give
exp(-200)), so the loss is 1/2 (1/N + 1/M) -- the diagonal alone -- and its
gradient is exactly zero: the reference's call trains nothing.
``batch_EMD_loss`` keeps that blur because it is what the reference computes;
a useful blur for clouds in the unit cube is 0.05 to 0.5.
"""
import os
import sys

import torch
from torch import nn
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402

KERNELS = {"gaussian": pcm_hip.KERNEL_GAUSSIAN, "laplacian": pcm_hip.KERNEL_LAPLACIAN,
           "energy": pcm_hip.KERNEL_ENERGY}


def _like(pts, lay):
    """An uninitialised tensor of the cloud's shape and layout."""
    return torch.empty_like(pts) if lay == 0 else torch.empty_like(pts.transpose(1, 2)).transpose(1, 2)


class kernel_lossFunction(Function):
    """``apply(x, y, kernel, blur)``: the [B] kernel norms of the float32
    clouds x [B, N, 3] and y [B, M, 3] (rows, or views of channel planes, read
    in place) for ``kernel`` in pcm_hip.KERNEL_*.  The unit gradients come from
    the one call in ``forward`` -- only those ``ctx.needs_input_grad`` asks
    for, in their cloud's layout -- and ``backward`` scales them by the
    upstream [B] gradient."""

    @staticmethod
    def forward(ctx, x, y, kernel, blur):
        for t in (x, y):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("the kernel loss expects float32 clouds")
            if t.dim() != 3 or t.size(2) != 3:
                raise ValueError("the kernel loss expects clouds [B, N, 3] and [B, M, 3]")
        if x.size(0) != y.size(0):
            raise ValueError("the kernel loss expects clouds of one batch size")
        if not (x.is_cuda and y.is_cuda):
            raise RuntimeError(f"the kernel loss needs HIP device tensors (got {x.device} and {y.device}); "
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
        pcm_hip.kernel_loss(p1, l1, p2, l2, int(kernel), float(blur), loss, g1, g2)
        ctx.save_for_backward(g1, g2)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        g1, g2 = ctx.saved_tensors
        w = grad_loss.reshape(-1, 1, 1)
        return (None if g1 is None else w * g1), (None if g2 is None else w * g2), None, None


class SamplesLoss(nn.Module):
    """geomloss's calling convention for unweighted clouds: ``SamplesLoss(loss,
    p, blur)(x, y)`` with x [N, 3] and y [M, 3] gives a scalar, with x
    [B, N, 3] and y [B, M, 3] one value per batch element.  ``loss`` is
    'gaussian', 'laplacian' or 'energy'; ``p`` is accepted and not used (it
    belongs to 'sinkhorn', which loss/sinkhorn_loss.py's SamplesLoss offers)."""

    def __init__(self, loss="gaussian", p=2, blur=0.05, **kwargs):
        super().__init__()
        if loss not in KERNELS:
            raise NotImplementedError(f"SamplesLoss(loss={loss!r}) is not offered here: the kernel norms "
                                      f"{sorted(KERNELS)} are (loss/sinkhorn_loss.py has 'sinkhorn')")
        if kwargs:
            raise NotImplementedError(f"SamplesLoss options {sorted(kwargs)} are not offered here")
        if not float(blur) > 0:
            raise ValueError("blur must be positive")
        self.loss, self.p, self.blur = loss, p, float(blur)

    def forward(self, *args):
        if len(args) != 2:
            raise NotImplementedError("weighted clouds (alpha, x, beta, y) are not offered here: SamplesLoss "
                                      "takes (x, y) with uniform weights")
        x, y = args
        if x.dim() == 2 and y.dim() == 2:
            return kernel_lossFunction.apply(x.unsqueeze(0), y.unsqueeze(0), KERNELS[self.loss], self.blur)[0]
        return kernel_lossFunction.apply(x, y, KERNELS[self.loss], self.blur)


def batch_EMD_loss(x, y):
    """loss/loss_.py:111-120: the mean over the batch of the Gaussian kernel
    norm at blur 5e-5 -- one library call in place of B Python iterations.  See
    the module docstring for what that blur does."""
    return torch.mean(SamplesLoss(loss="gaussian", p=2, blur=.00005)(x, y))
