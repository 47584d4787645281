"""Sampling and grouping with pointnet2's calling convention -- the
``pointnet2_ops.pointnet2_utils`` (``pn2_utils``) that the reference's dropped
``get_uniform_loss`` called: ``furthest_point_sample``, ``gather_operation``,
``ball_query`` and ``grouping_operation``.

``pointnet2_ops`` is not installed here and could not be fetched, so nothing in
this module has been compared against it.  The interface is taken from the
call sites and from pointnet2's published source; the ball query's rule -- a
point is a hit when its squared distance is strictly below radius squared, a
list is the first ``nsample`` hits in index order, the remaining slots repeat
the first hit and a ball without a hit is all zeros -- is stated from that
source, unverified.  include/pcm.h has it as the contract of pcm_ball_query
(csrc/grouping.hip), which is what runs here, one launch per call.

Differences:
  * clouds are float32 [B, N, 3] on a HIP device with at most
    pcm_hip.KNN_MAX_POINTS points and ``nsample`` <= pcm_hip.BALL_MAX_NSAMPLE:
    all compute goes through libpcm_hip.so and CPU tensors raise;
  * a [B, N, 3] view of contiguous [B, 3, N] planes is read in place
    (pcm_hip.cloud_layout); other strides are made contiguous first;
  * distances are formed in the library's pinned order fma(dz, dz, fma(dy, dy,
    dx * dx)), where pointnet2 sums three squares: a point within a few float32
    ulps of the sphere may fall on the other side;
  * ``furthest_point_sample`` is pcm_fps started at point 0, as pointnet2's is;
  * the two gathers are torch indexing (as sampling.index_points), on any
    device, differentiable in ``features``; the index outputs carry no gradient;
  * ``ball_query_count`` also returns how many slots of each list are hits.
"""
import os
import sys

import torch

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


def _cloud(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"pointnet2_utils expects float32 clouds ({name})")
    if t.dim() != 3 or t.size(2) != 3:
        raise ValueError(f"pointnet2_utils expects clouds [B, N, 3] ({name})")
    if not t.is_cuda:
        raise RuntimeError(f"pointnet2_utils needs HIP device tensors (got {name} on {t.device}); "
                           "there is no CPU path")
    t = t.detach()
    lay = pcm_hip.cloud_layout(t)
    if lay is None:
        t, lay = t.contiguous(), 0
    return t, lay


def furthest_point_sample(xyz, npoint):
    """int32 [B, npoint] indices of the farthest point samples of ``xyz``
    [B, N, 3], every cloud started at point 0: one pcm_fps launch."""
    npoint = int(npoint)
    if npoint < 1:
        raise ValueError("npoint must be at least 1")
    xyz, lay = _cloud(xyz, "xyz")
    idx = torch.empty(xyz.size(0), npoint, dtype=torch.long, device=xyz.device)
    pcm_hip.fps(xyz, lay, npoint, 0, idx)
    return idx.int()


def gather_operation(features, idx):
    """``features`` [B, C, N] and integer ``idx`` [B, S] -> [B, C, S] holding
    ``features[b, :, idx[b, s]]``; differentiable in ``features``."""
    if features.dim() != 3 or idx.dim() != 2 or idx.size(0) != features.size(0):
        raise ValueError("gather_operation expects features [B, C, N] and idx [B, S]")
    pick = idx.long().unsqueeze(1).expand(-1, features.size(1), -1)
    return torch.gather(features, 2, pick)


def ball_query_count(radius, nsample, xyz, new_xyz):
    """(idx, cnt) of one pcm_ball_query launch: idx int32 [B, S, nsample] as
    ``ball_query`` returns it and cnt int32 [B, S], the number of leading slots
    that are hits (the rest is padding)."""
    nsample = int(nsample)
    if nsample < 1:
        raise ValueError("nsample must be at least 1")
    xyz, lay_x = _cloud(xyz, "xyz")
    new_xyz, lay_c = _cloud(new_xyz, "new_xyz")
    if new_xyz.size(0) != xyz.size(0):
        raise ValueError("xyz and new_xyz differ in batch size")
    b, s = new_xyz.size(0), new_xyz.size(1)
    idx = torch.empty(b, s, nsample, dtype=torch.int32, device=xyz.device)
    cnt = torch.empty(b, s, dtype=torch.int32, device=xyz.device)
    pcm_hip.ball_query(xyz, lay_x, new_xyz, lay_c, float(radius), nsample, idx, cnt)
    return idx, cnt


def ball_query(radius, nsample, xyz, new_xyz):
    """int32 [B, S, nsample]: for every centre of ``new_xyz`` [B, S, 3] the
    first ``nsample`` points of ``xyz`` [B, N, 3], in index order, strictly
    inside the ball of ``radius``; the remaining slots repeat the first hit, and
    a ball without a hit is all zeros."""
    return ball_query_count(radius, nsample, xyz, new_xyz)[0]


def grouping_operation(features, idx):
    """``features`` [B, C, N] and integer ``idx`` [B, S, K] -> [B, C, S, K]
    holding ``features[b, :, idx[b, s, k]]``; differentiable in ``features``."""
    if features.dim() != 3 or idx.dim() != 3 or idx.size(0) != features.size(0):
        raise ValueError("grouping_operation expects features [B, C, N] and idx [B, S, K]")
    b, c = features.size(0), features.size(1)
    s, k = idx.size(1), idx.size(2)
    pick = idx.long().reshape(b, 1, s * k).expand(-1, c, -1)
    return torch.gather(features, 2, pick).reshape(b, c, s, k)
