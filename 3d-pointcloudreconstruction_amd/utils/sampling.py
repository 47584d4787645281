"""Farthest point sampling -- working counterpart of ``farthest_point_sample``
and ``index_points`` in the reference's utils/utils.py:316-360, which
utils/datasets_sample_pcl.py:87-94 calls to make the 128- and 256-point ground
truth of the coarse-to-fine generator.

The module is ``sampling``, not ``utils``: this directory is on ``sys.path``
next to the package root, and a ``utils.py`` inside it would shadow it.

``farthest_point_sample`` is the hot one.  The reference runs ``npoint``
dependent iterations of 21 small device kernels each (torch.profiler's count,
DESIGN.md section 3.13), with a boolean-mask assignment that synchronises with the host every iteration.  Here
it is one launch of pcm_fps (csrc/sampling.hip): one workgroup per cloud, the
running minima in registers for the whole call; include/pcm.h has the contract.

Differences:
  * clouds are float32 [B, N, 3] with N <= pcm_hip.FPS_MAX_POINTS, on a HIP
    device: all compute goes through libpcm_hip.so and CPU tensors raise;
  * a [B, N, 3] view of contiguous [B, 3, N] planes is read in place
    (pcm_hip.cloud_layout); other strides are made contiguous first;
  * the start index is written down, not drawn: ``torch.randint(0, 1)`` and
    ``torch.randint(1, 2)`` (utils.py:347-350) can only return 0 and 1, so
    ``RAN=True`` starts every cloud at point 0 and ``RAN=False`` at point 1;
    ``RAN=False`` on one-point clouds raises ValueError (the reference:
    IndexError);
  * distances are formed in the library's pinned order fma(dz, dz, fma(dy, dy,
    dx * dx)); the reference's torch sum can differ in the last bits, which
    changes a pick only where two running minima are within a few ulps;
  * ``sample_points`` returns the indices and the gathered points from the one
    launch.
"""
import os
import sys

import torch

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


def _sample(xyz, npoint, RAN, want_points):
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32:
        raise TypeError("farthest point sampling expects a float32 cloud")
    if xyz.dim() != 3 or xyz.size(2) != 3:
        raise ValueError("farthest point sampling expects a cloud [B, N, 3]")
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError("npoint must be at least 1")
    start = 0 if RAN else 1
    if start >= xyz.size(1):
        raise ValueError(f"RAN=False starts at point 1: the cloud needs two points (got {xyz.size(1)})")
    if not xyz.is_cuda:
        raise RuntimeError(f"farthest point sampling needs a HIP device tensor (got one on {xyz.device}); "
                           "there is no CPU path")
    xyz = xyz.detach()
    lay = pcm_hip.cloud_layout(xyz)
    if lay is None:
        xyz, lay = xyz.contiguous(), 0
    b = xyz.size(0)
    idx = torch.empty(b, npoint, dtype=torch.long, device=xyz.device)
    new_xyz = torch.empty(b, npoint, 3, dtype=torch.float32, device=xyz.device) if want_points else None
    pcm_hip.fps(xyz, lay, npoint, start, idx, new_xyz)
    return idx, new_xyz


def farthest_point_sample(xyz, npoint, RAN=True):
    """Indices of ``npoint`` farthest point samples per cloud, as a torch.long
    tensor [B, npoint] on ``xyz``'s device: one pcm_fps launch.  ``xyz`` is a
    float32 [B, N, 3] tensor on a HIP device; every cloud starts at point 0
    (``RAN=True``) or at point 1 (``RAN=False``), and each further pick is the
    lowest-numbered point farthest from all picks so far.  ``npoint`` above N
    is allowed (include/pcm.h says what repeats)."""
    return _sample(xyz, npoint, RAN, False)[0]


def index_points(points, idx):
    """Gather rows of a batch by per-batch indices: for ``points`` of shape
    [B, N, C] and integer ``idx`` of shape [B, S] or [B, S, K], the result has
    ``idx``'s shape with C appended and holds ``points[b, idx[b, ...], :]``.
    Plain torch indexing on any device, differentiable in ``points``."""
    b = points.shape[0]
    view = [b] + [1] * (idx.dim() - 1)
    batch = torch.arange(b, dtype=torch.long, device=points.device).view(view).expand(idx.shape)
    return points[batch, idx.to(points.device), :]


def sample_points(xyz, npoint, RAN=True):
    """(idx, new_xyz) from one launch: idx as farthest_point_sample, new_xyz
    float32 [B, npoint, 3] equal to index_points(xyz, idx) bit for bit.  new_xyz
    is detached: no gradient flows to xyz (use index_points(xyz, idx) for one)."""
    return _sample(xyz, npoint, RAN, True)
