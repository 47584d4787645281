"""Evaluation-loss glue -- working counterpart of the reference's loss/loss_.py.

Same function names and signatures (loss/loss_.py:9-13, :79-109, :122-140):
``cd``, ``distChamfer``, ``batch_NN_loss`` and ``fscore``.  The reference
resolves ``dist_chamfer_3D`` relative to the working directory (:6); here it
is resolved relative to this file.  ``batch_EMD_loss`` (:111-120), which the
reference builds on the third-party geomloss package, lives in
loss/kernel_loss.py with the kernel norms it needs.

Differences:
  * ``distChamfer`` / ``batch_NN_loss`` build no B x N x M float64 matrix
    (:66-77): they run the Chamfer forward (float32, the pinned evaluation
    order of chamfer3D.cu), so their values are the reference's to float32
    rounding, not float64;
  * ``fscore`` is ONE pcm_chamfer_eval call (csrc/chamfer_eval.hip): no
    per-point output, no torch reductions.  Its batch means are sequential
    float32 sums over the clouds.
All compute goes through libpcm_hip.so; CPU tensors raise.
"""
import os
import sys

import torch

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
_p = os.path.join(_METRIC, "chamfer3D")
if _p not in sys.path:
    sys.path.append(_p)
from dist_chamfer_3D import chamfer_3DDist  # noqa: E402
from eval_chamfer_3D import chamfer_eval_batch  # noqa: E402


def cd(fake, points):
    """mean(dist1) + mean(dist2) (squared L2), loss_.py:9-13."""
    dist1, dist2, idx1, idx2 = chamfer_3DDist()(fake, points)
    return torch.mean(dist1) + torch.mean(dist2)


def distChamfer(a, b):
    """loss_.py:79-91: (closest squared distance in b of every point of a,
    closest in a of every point of b, and the two argmins as int32)."""
    return chamfer_3DDist()(a, b)


def batch_NN_loss(x, y):
    """loss_.py:93-109: (mean(mins1) + mean(mins2), mins1, mins2), where mins1
    [B, M] is the distance of every point of y to x (the forward's dist2) and
    mins2 [B, N] the distance of every point of x to y (its dist1)."""
    dist1, dist2, _, _ = chamfer_3DDist()(x, y)
    mins1, mins2 = dist2, dist1
    return torch.mean(mins1) + torch.mean(mins2), mins1, mins2


def fscore(X, Y, threshold=0.0001):
    """loss_.py:122-140: (fscore, precision_1, precision_2) at a squared-distance
    threshold, three 0-dim float32 tensors: the batch means of the per-cloud
    F-score, of the share of Y's points within the threshold of X (precision_1)
    and of the share of X's points within the threshold of Y (precision_2).
    A cloud pair with no point under the threshold scores 0 (:135)."""
    _, batch = chamfer_eval_batch(X, Y, (threshold,))
    f = batch[0, 0].requires_grad_()  # as :139
    return f, batch[0, 2], batch[0, 1]


if __name__ == "__main__":
    images_1 = torch.rand(32, 1024, 3).cuda()
    images_2 = torch.rand(32, 1024, 3).cuda()
    print(cd(images_1, images_2))
    print(fscore(images_1, images_2, 0.001))
