"""Cross Chamfer matrix: the Chamfer distance of every cloud of one set to
every cloud of another, in one call.

Every other Chamfer entry of this package pairs cloud b of one batch with
cloud b of the other.  Nearest-shape retrieval, the set-level metrics MMD-CD,
COV-CD and 1-NNA-CD (utils/set_metrics.py) and duplicate checks between a
training and a test split all need the S x R matrix instead.
``chamfer_cross(x, y)`` runs pcm_chamfer_cross (csrc/chamfer_cross.hip): a
workgroup keeps a block of one cloud's points in registers and streams a run
of the other set's clouds past them, so nothing is copied or expanded and the
whole matrix costs at most two launches.

The per-point distances behind the means are exactly chamfer_3DDist's dist1 /
dist2 of that pair of clouds (float32, the pinned evaluation order); a cloud's
points are added in float64 and the mean is rounded to float32 once.  Entry
(i, j) depends on x[i] and y[j] alone, bit for bit.  Outputs carry no autograd
history: this is a metric.  float32 clouds on a HIP device only; CPU tensors
raise.  Clouds of up to pcm_hip.CROSS_MAX_POINTS points.
"""
import collections
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcm_hip  # noqa: E402

# mean12[i, j]: mean over x[i]'s points of the squared distance to the nearest point of y[j];
# mean21[i, j]: mean over y[j]'s points of the squared distance to the nearest point of x[i];
# cd = mean12 + mean21, all [S, R]
ChamferCross = collections.namedtuple("ChamferCross", ["mean12", "mean21", "cd"])


def _check_sets(*sets):
    """Shapes, then dtypes, then devices, of every set before anything runs."""
    for t in sets:
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.size(2) != 3:
            raise ValueError("chamfer_cross expects cloud sets of shape [S, N, 3] and [R, M, 3]")
    for t in sets:
        if t.dtype != torch.float32:
            raise TypeError(f"chamfer_cross expects float32 clouds (got {t.dtype})")
    for t in sets:
        if t.device.type != "cuda":
            raise RuntimeError(
                f"chamfer_cross needs HIP device tensors (got a tensor on {t.device}); there is no CPU path")
        if t.device != sets[0].device:
            raise RuntimeError(f"tensors on different devices: {sets[0].device} vs {t.device}")


def _cloud_set(t):
    t = t.detach()
    lay = pcm_hip.cloud_layout(t)
    if lay is None:  # neither rows nor a view of channel planes
        t = t.contiguous()
        lay = 0
    return t, lay


def chamfer_cross(x, y=None):
    """ChamferCross(mean12, mean21, cd) of [S, R] float32 tensors for the cloud
    sets x [S, N, 3] and y [R, M, 3].  Views of channel planes ([S, 3, N]
    transposed) are read in place.  y=None compares x with itself: one
    direction is computed, mean21 = mean12^T and cd = mean12 + mean12^T -- half
    the work, exactly symmetric, with a diagonal of exactly 0; bit for bit what
    chamfer_cross(x, x) returns."""
    _check_sets(*((x,) if y is None else (x, y)))
    xs, lay_x = _cloud_set(x)
    if y is None:
        s = xs.size(0)
        mean12 = torch.empty(s, s, device=xs.device)
        pcm_hip.chamfer_cross(xs, lay_x, xs, lay_x, mean12)
        mean21 = mean12.t()
        return ChamferCross(mean12, mean21, mean12 + mean21)
    ys, lay_y = _cloud_set(y)
    s, r = xs.size(0), ys.size(0)
    mean12 = torch.empty(s, r, device=xs.device)
    mean21 = torch.empty(s, r, device=xs.device)
    pcm_hip.chamfer_cross(xs, lay_x, ys, lay_y, mean12, mean21)
    return ChamferCross(mean12, mean21, mean12 + mean21)


class chamfer_3DCross(nn.Module):
    """``chamfer_3DCross()(x, y=None)`` -> ChamferCross named tuple (mean12,
    mean21, cd), each [S, R], on the inputs' device."""

    def forward(self, x, y=None):
        return chamfer_cross(x, y)
