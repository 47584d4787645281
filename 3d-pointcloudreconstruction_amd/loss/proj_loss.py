"""Projection loss -- working counterpart of the reference's loss/proj_loss.py.

Same function names and signatures (proj_loss.py:6-43, :46-54):
``get_loss_proj`` and ``grid_dist``.  finetune.py:158 calls
``get_loss_proj(proj_pred, proj_gt, 'cuda', 'bce_prob', 1.0, True,
grid_dist_tensor, opt=opt)`` on the two silhouettes of utils/projection.py's
``cont_proj``.

``'bce_prob'`` (:17-19 and the mean of :43) is ONE pcm_proj_bce call behind an
autograd Function (csrc/silhouette.hip): the loss and its gradient for
``pred`` from the same launch, where the reference runs six elementwise torch
kernels, a reduction and their autograd backward.  ``'bce'`` and
``'weighted_bce'`` are the reference's two torch losses with its argument
order, ``(gt, pred)``.

Differences:
  * no ``.cuda()`` on the result: it stays on the inputs' device; nothing is
    printed;
  * with ``min_dist_loss=None`` the last two values are ``None`` (the
    reference raises NameError there);
  * ``dist_mat`` is not modified in place (the reference adds 1 to the
    caller's tensor on every call); a numpy table, as ``grid_dist`` returns
    it, is accepted as well as a tensor; ``opt`` is not needed (the grid is
    ``dist_mat``'s);
  * no [B, H, W, H, W] tensor is built.  The reference broadcasts both ``gt``
    and ``pred`` over the last two axes (:25-29), so with D = dist_mat + 1
    its minima over those axes are, per cell, a product of three numbers of
    which only D[i, j, k, l] varies: the minimum is taken at min_kl D[i, j]
    where the other two factors' signs agree and at max_kl D[i, j] where they
    differ (a float32 product is monotone in each factor).  The two [H, W]
    extrema of D are computed once, with torch;
  * ``'bce_prob'`` goes through libpcm_hip.so: CPU tensors raise, float32 only;
  * ``grid_dist`` needs no scipy.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


class proj_bce_probFunction(Function):
    """mean(-gt log(pred + 1e-8) w - (1 - gt) log|1 - pred - 1e-8|), float32,
    in the pinned order of include/pcm.h; differentiable in ``pred``."""

    @staticmethod
    def forward(ctx, pred, gt, w):
        if pred.dtype != torch.float32 or gt.dtype != torch.float32:
            raise TypeError("the 'bce_prob' projection loss expects float32 silhouettes")
        if pred.shape != gt.shape:
            raise ValueError("pred and gt silhouettes differ in shape")
        pred_c, gt_c = pred.contiguous(), gt.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        if pred.numel() == 0:
            loss.fill_(float("nan"))  # the mean over nothing, as torch.mean's
        grad = torch.empty_like(pred_c) if ctx.needs_input_grad[0] else None
        pcm_hip.proj_bce(pred_c, gt_c, w, loss, grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return grad_loss * grad, None, None


def _extreme_at(coef_a, coef_b, d_min, d_max):
    """min over (k, l) of (coef_a * D[i, j, k, l]) * coef_b per batch element
    and cell (i, j), in the reference's order of operations."""
    same = torch.sign(coef_a) * torch.sign(coef_b) >= 0
    return torch.where(same, (coef_a * d_min) * coef_b, (coef_a * d_max) * coef_b)


def get_loss_proj(pred, gt, device=None, loss_type='bce', w=1., min_dist_loss=None, dist_mat=None, opt=None):
    """proj_loss.py:6-43: (loss, min_dist, min_dist_inv) for the predicted and
    ground-truth silhouettes [B, H, W]; ``dist_mat`` is grid_dist's [H, W, H, W]
    table.  ``device`` is accepted for signature compatibility."""
    if loss_type == 'bce':
        loss = nn.BCELoss()(gt, pred)
    elif loss_type == 'weighted_bce':
        loss = nn.BCEWithLogitsLoss()(gt, pred)
    elif loss_type == 'bce_prob':
        loss = proj_bce_probFunction.apply(pred, gt.detach(), float(w))
    else:
        raise ValueError("loss_type must be 'bce', 'weighted_bce' or 'bce_prob' (got %r)" % (loss_type,))

    min_dist = min_dist_inv = None
    if min_dist_loss is not None:
        D = torch.as_tensor(dist_mat).to(device=pred.device, dtype=pred.dtype) + 1
        d_min = D.flatten(2).min(2)[0]  # [H, W]
        d_max = D.flatten(2).max(2)[0]
        pred_mask = pred + (1. - pred) * 1e6
        gt_th = gt + (1. - gt) * 1e6
        min_dist = _extreme_at(gt_th, pred, d_min, d_max)
        min_dist_inv = _extreme_at(gt, pred_mask, d_min, d_max)
    return loss, min_dist, min_dist_inv  # every loss above is already the mean of :43


def grid_dist(grid_h, grid_w):
    """proj_loss.py:46-54: the Euclidean distance between every two cells of
    the grid, a float64 numpy array [grid_h, grid_w, grid_h, grid_w]."""
    x, y = np.meshgrid(np.arange(grid_h, dtype=np.float64), np.arange(grid_w, dtype=np.float64), indexing='ij')
    dx = x[:, :, None, None] - x[None, None, :, :]
    dy = y[:, :, None, None] - y[None, None, :, :]
    return np.sqrt(dx * dx + dy * dy)
