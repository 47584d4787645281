"""Chamfer evaluation module: F-score, precision and recall at squared-distance
thresholds, and the per-cloud mean nearest-neighbour distances, in one pass.

The evaluation-side companion of dist_chamfer_3D.py.  The reference computes
the F-score (loss/loss_.py:122-140) from batch_NN_loss's float64 B x N x M
distance matrix (:93-109) and six torch reductions per threshold; with this
project's chamfer_3DDist it would still take the argmin forward, four per-point
arrays and those reductions.  ``chamfer_3DEval(thresholds)(xyz1, xyz2)`` runs
pcm_chamfer_eval instead (csrc/chamfer_eval.hip): a distance-only scan of both
directions whose epilogue counts the points under every threshold, then a tiny
finalising launch.  Up to eight thresholds cost one pass.

The per-point distances behind the counts are exactly chamfer_3DDist's dist1 /
dist2 (float32, the pinned evaluation order), and ``<`` is strict as in
loss_.py:132-133.  Outputs carry no autograd history (the reference's F-score
has no usable gradient either: a comparison stands between it and the clouds).
Same dtype rules as chamfer_3DFunction: float32 or float16 clouds of one
dtype; CPU tensors raise.
"""
import collections
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcm_hip  # noqa: E402

# precision = p_x: the share of input1's points within the threshold of input2;
# recall = p_y: the share of input2's points within the threshold of input1
ChamferEval = collections.namedtuple(
    "ChamferEval", ["mean_dist1", "mean_dist2", "count1", "count2", "precision", "recall", "fscore"])


def chamfer_eval_batch(input1, input2, thresholds):
    """(ChamferEval of per-cloud values, batch_scores [T, 3]) from ONE
    pcm_chamfer_eval call; batch_scores[t] = the batch means of (F-score, p_x,
    p_y) at thresholds[t], summed over the clouds in ascending order."""
    thresholds = tuple(float(t) for t in thresholds)
    if input1.dim() != 3 or input2.dim() != 3 or input1.size(2) != 3 or input2.size(2) != 3:
        raise ValueError("chamfer_3DEval expects clouds [B, N, 3] and [B, M, 3]")
    if input2.size(0) != input1.size(0):
        raise ValueError("batch sizes of the two clouds differ")
    if input1.dtype != input2.dtype or input1.dtype not in (torch.float32, torch.float16):
        raise TypeError("chamfer_3DEval expects float32 (or float16) clouds of one dtype")
    xyz1 = input1.detach().contiguous()
    xyz2 = input2.detach().contiguous()
    b, t = xyz1.size(0), len(thresholds)
    dev = xyz1.device
    mean_dist = torch.empty(b, 2, device=dev)
    counts = torch.empty(b, t, 2, dtype=torch.int32, device=dev)
    scores = torch.empty(b, t, 3, device=dev)
    # the mean over an empty batch is not a number, as torch.mean's
    batch = torch.empty(t, 3, device=dev) if b > 0 else torch.full((t, 3), float("nan"), device=dev)
    pcm_hip.chamfer_eval(xyz1, xyz2, thresholds, mean_dist, counts, scores, batch)
    per_cloud = ChamferEval(mean_dist[:, 0], mean_dist[:, 1], counts[:, :, 0], counts[:, :, 1],
                            scores[:, :, 1], scores[:, :, 2], scores[:, :, 0])
    return per_cloud, batch


class chamfer_3DEval(nn.Module):
    """``chamfer_3DEval(thresholds)(input1, input2)`` -> ChamferEval named tuple
    (mean_dist1 [B], mean_dist2 [B], count1 [B,T] int32, count2 [B,T] int32,
    precision [B,T], recall [B,T], fscore [B,T]) on the inputs' device, for
    1..8 squared-distance thresholds (a float or a sequence, in any order)."""

    def __init__(self, thresholds=(0.0001,)):
        super(chamfer_3DEval, self).__init__()
        if isinstance(thresholds, (int, float)):
            thresholds = (thresholds,)
        self.thresholds = tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= pcm_hip.EVAL_MAX_THRESHOLDS:
            raise ValueError("chamfer_3DEval takes 1..%d thresholds" % pcm_hip.EVAL_MAX_THRESHOLDS)

    def forward(self, input1, input2):
        return chamfer_eval_batch(input1, input2, self.thresholds)[0]

    def batch_means(self, input1, input2):
        """[T, 3] batch means of (F-score, precision, recall), loss_.py:136-138."""
        return chamfer_eval_batch(input1, input2, self.thresholds)[1]
