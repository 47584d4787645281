"""Sliced 2-Wasserstein distance between two point clouds (Nguyen et al.,
"Point-set distances for learning representations of 3D point clouds"): the
mean over L directions of the exact 1-D transport cost between the clouds'
projections,

    SW(x, y) = (1/L) sum_l W2^2(theta_l . x, theta_l . y),   masses 1/N and 1/M.

The whole batch is ONE pcm_sliced_wasserstein_loss call behind an autograd
Function (csrc/sliced.hip; include/pcm.h has the contract): project, sort in a
pinned total order, match the sorted lists.  It is a transport loss at
O(L N log N) cost, defined for any N and M (N != M included), differentiable in
both clouds and exact per slice -- no epsilon, no schedule, no iteration count.

The directions are taken as given: ``sliced_directions`` draws random unit
vectors or the deterministic Fibonacci lattice.  A fixed ``directions`` tensor
keeps the call free of random draws and capturable in a graph.
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

KINDS = ("random", "fibonacci")


def _like(pts, lay):
    """An uninitialised tensor of the cloud's shape and layout."""
    return torch.empty_like(pts) if lay == 0 else torch.empty_like(pts.transpose(1, 2)).transpose(1, 2)


def sliced_directions(L, device=None, generator=None, kind="random"):
    """[L, 3] float32 unit directions on ``device``.  ``kind='random'``:
    ``randn`` rows (drawn with ``generator`` on the generator's device, else on
    ``device``), normalised.  ``kind='fibonacci'``: the Fibonacci lattice of L
    points on the sphere, z_k = 1 - (2 k + 1) / L at the golden angle, computed
    in float64 on the host -- the same bits everywhere, for evaluation."""
    L = int(L)
    if not 1 <= L <= pcm_hip.SLICED_MAX_DIRS:
        raise ValueError(f"the number of directions must lie in [1, {pcm_hip.SLICED_MAX_DIRS}] (got {L})")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
    if kind == "fibonacci":
        k = torch.arange(L, dtype=torch.float64)
        z = 1.0 - (2.0 * k + 1.0) / L
        r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
        phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
        d = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], dim=1).to(torch.float32)
        return d.to(device) if device is not None else d
    where = generator.device if generator is not None else device
    d = torch.randn(L, 3, dtype=torch.float32, device=where, generator=generator)
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return d.to(device) if device is not None else d


class sliced_wassersteinFunction(Function):
    """``apply(x, y, directions)``: the [B] sliced Wasserstein distances of the
    float32 clouds x [B, N, 3] and y [B, M, 3] (rows, or views of channel
    planes, read in place) over the float32 directions [L, 3], and the [B, L]
    per-slice values (not differentiable).  The unit gradients come from the
    one call in ``forward`` -- only those ``ctx.needs_input_grad`` asks for, in
    their cloud's layout -- and ``backward`` scales them by the upstream [B]
    gradient."""

    @staticmethod
    def forward(ctx, x, y, directions):
        for t in (x, y):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("the sliced Wasserstein loss expects float32 clouds")
            if t.dim() != 3 or t.size(2) != 3:
                raise ValueError("the sliced Wasserstein loss expects clouds [B, N, 3] and [B, M, 3]")
        if x.size(0) != y.size(0):
            raise ValueError("the sliced Wasserstein loss expects clouds of one batch size")
        if not isinstance(directions, torch.Tensor) or directions.dtype != torch.float32:
            raise TypeError("the sliced Wasserstein loss expects float32 directions")
        if directions.dim() != 2 or directions.size(1) != 3 or directions.size(0) == 0:
            raise ValueError("the sliced Wasserstein loss expects directions [L, 3]")
        if not (x.is_cuda and y.is_cuda and directions.is_cuda):
            raise RuntimeError(f"the sliced Wasserstein loss needs HIP device tensors (got {x.device}, {y.device} "
                               f"and {directions.device}); there is no CPU path")
        clouds = []
        for t in (x, y):
            pts = t.detach()
            lay = pcm_hip.cloud_layout(pts)
            if lay is None:
                pts, lay = pts.contiguous(), 0
            clouds.append((pts, lay))
        (p1, l1), (p2, l2) = clouds
        dirs = directions.detach().contiguous()
        loss = torch.empty(p1.size(0), dtype=torch.float32, device=p1.device)
        slices = torch.empty(p1.size(0), dirs.size(0), dtype=torch.float32, device=p1.device)
        g1 = _like(p1, l1) if ctx.needs_input_grad[0] else None
        g2 = _like(p2, l2) if ctx.needs_input_grad[1] else None
        pcm_hip.sliced_wasserstein_loss(p1, l1, p2, l2, dirs, loss, slices, g1, g2)
        ctx.save_for_backward(g1, g2)
        ctx.mark_non_differentiable(slices)
        return loss, slices

    @staticmethod
    def backward(ctx, grad_loss, _grad_slices):
        g1, g2 = ctx.saved_tensors
        w = grad_loss.reshape(-1, 1, 1)
        return (None if g1 is None else w * g1), (None if g2 is None else w * g2), None


class SlicedWassersteinLoss(nn.Module):
    """``SlicedWassersteinLoss(n_projections, directions, generator, kind)(x,
    y)``: with x [N, 3] and y [M, 3] a scalar, with x [B, N, 3] and y
    [B, M, 3] one value per batch element; ``return_slices=True`` also gives
    the [B, L] (or [L]) per-slice values.

    ``directions=None`` draws ``n_projections`` directions of ``kind`` on every
    call (``generator`` seeds the random ones; the Fibonacci lattice is the
    same every time).  A fixed ``directions`` tensor [L, 3] is used as given --
    not normalised -- and keeps the call capturable in a graph."""

    def __init__(self, n_projections=128, directions=None, generator=None, kind="random", return_slices=False):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
        if directions is not None:
            if not isinstance(directions, torch.Tensor) or directions.dim() != 2 or directions.size(1) != 3:
                raise ValueError("directions must be a tensor [L, 3]")
            n_projections = directions.size(0)
        if not 1 <= int(n_projections) <= pcm_hip.SLICED_MAX_DIRS:
            raise ValueError(f"n_projections must lie in [1, {pcm_hip.SLICED_MAX_DIRS}] (got {n_projections})")
        self.n_projections, self.directions, self.generator, self.kind = int(n_projections), directions, generator, kind
        self.return_slices = bool(return_slices)

    def forward(self, x, y, return_slices=None):
        single = x.dim() == 2 and y.dim() == 2
        if single:
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        dirs = self.directions
        if dirs is None:
            if not (x.is_cuda and y.is_cuda):
                raise RuntimeError(f"the sliced Wasserstein loss needs HIP device tensors (got {x.device} and "
                                   f"{y.device}); there is no CPU path")
            dirs = sliced_directions(self.n_projections, x.device, self.generator, self.kind)
        loss, slices = sliced_wassersteinFunction.apply(x, y, dirs)
        if single:
            loss, slices = loss[0], slices[0]
        want = self.return_slices if return_slices is None else return_slices
        return (loss, slices) if want else loss
