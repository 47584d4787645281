"""Silhouette projection -- working counterpart of the reference's utils/projection.py.

Same module and function names as the four the reference's utils/utils.py:7
imports: ``cont_proj``, ``apply_kernel``, ``perspective_transform`` and
``world2cam`` (projection.py:4-67, :97-108, :110-146, :148-199).  Left out:
``disc_proj`` and the cloud-editing helpers ``scale2one`` / ``average_pcl`` /
``outlier``.

``cont_proj`` is the hot one.  The reference builds a B x N x H x W x 2
float32 difference tensor, its exponential, a B x N x H x W product and a sum
over N (32 MiB per cloud per tensor at N=1024, 64x64), and moves the work to
the CPU to do it (utils/utils.py:232).  Here it is an autograd Function over
pcm_silhouette_forward / pcm_silhouette_backward (csrc/silhouette.hip): one
launch each way, nothing of size N x H x W anywhere.

Differences:
  * ``cont_proj``'s result lives on ``pcl``'s device; ``device`` is accepted for
    signature compatibility and otherwise ignored (the reference moves the
    work to ``device``).  All compute goes through libpcm_hip.so: CPU tensors
    raise, and clouds are float32 (the dtype rule of chamfer_3DFunction,
    without its float16 extension);
  * a [B, N, 3] view of contiguous [B, 3, N] planes -- what
    ``perspective_transform`` returns -- is read in place and its gradient
    written in the same layout (pcm_hip.cloud_layout);
  * grids up to pcm_hip.SILHOUETTE_MAX_GRID per side;
  * ``perspective_transform`` and ``world2cam`` follow their input's device
    (the reference's ``world2cam`` ends in ``.cuda()``); ``batch_size``,
    ``device`` and ``N_PTS`` are accepted and the shapes taken from ``xyz``.
"""
import os
import sys

import torch
from torch.autograd import Function

_METRIC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metric")
if _METRIC not in sys.path:
    sys.path.append(_METRIC)
import pcm_hip  # noqa: E402


class cont_projFunction(Function):
    """sil [B, H, W] = sum_n exp(-(gx_n - h)^2 / (2 s)) exp(-(gy_n - w)^2 / (2 s))
    with gx = (x + 1) H / 2, gy = (y + 1) W / 2 (include/pcm.h)."""

    @staticmethod
    def forward(ctx, pcl, grid_h, grid_w, sigma_sq):
        if pcl.dim() != 3 or pcl.size(2) != 3:
            raise ValueError("cont_proj expects a cloud [B, N, 3]")
        if pcl.dtype != torch.float32:
            raise TypeError("cont_proj expects a float32 cloud")
        lay = pcm_hip.cloud_layout(pcl) if pcl.is_cuda else 0
        if lay is None:
            pcl, lay = pcl.contiguous(), 0
        sil = torch.empty(pcl.size(0), int(grid_h), int(grid_w), dtype=torch.float32, device=pcl.device)
        pcm_hip.silhouette_forward(pcl, lay, grid_h, grid_w, sigma_sq, sil)
        ctx.save_for_backward(pcl)
        ctx.args = (lay, int(grid_h), int(grid_w), float(sigma_sq))
        return sil

    @staticmethod
    def backward(ctx, grad_sil):
        (pcl,) = ctx.saved_tensors
        lay, grid_h, grid_w, sigma_sq = ctx.args
        b, n, _ = pcl.shape
        if lay == 1:
            gradxyz = torch.empty(b, 3, n, dtype=torch.float32, device=pcl.device).transpose(1, 2)
        else:
            gradxyz = torch.empty(b, n, 3, dtype=torch.float32, device=pcl.device)
        g = grad_sil if grad_sil.dtype == torch.float32 else grad_sil.float()
        pcm_hip.silhouette_backward(pcl, lay, grid_h, grid_w, sigma_sq, g.contiguous(), gradxyz)
        return gradxyz, None, None, None


def cont_proj(pcl, grid_h, grid_w, device=None, sigma_sq=0.5):
    """projection.py:4-67: the continuous silhouette [B, grid_h, grid_w] of
    pcl [B, N, 3] (values assumed in (-1, 1); any value is legal), float32,
    differentiable, on pcl's device (``device`` is ignored)."""
    return cont_projFunction.apply(pcl, grid_h, grid_w, sigma_sq)


def apply_kernel(x, sigma_sq=0.5):
    """projection.py:97-108: the un-normalised Gaussian exp(-x^2 / (2 sigma_sq))."""
    return torch.exp(-(x ** 2) / (2. * sigma_sq))


def perspective_transform(xyz, device=None, batch_size=None):
    """projection.py:110-146: camera -> pixel co-ordinates with the intrinsics
    K = [[120, 0, -32], [0, 120, -32], [0, 0, 1]] of the 64 x 64 renderer:
    q = K p per point, then (q_x / |p_z|, q_y / |p_z|, |q_z|).  Returns the
    [B, N, 3] view of the [B, 3, N] planes it computes (on xyz's device)."""
    K = torch.tensor([[120., 0., -32.], [0., 120., -32.], [0., 0., 1.]], dtype=torch.float32, device=xyz.device)
    q = torch.matmul(K.unsqueeze(0).expand(xyz.size(0), 3, 3), xyz.permute(0, 2, 1))  # [B, 3, N]
    xy = q[:, :2] / torch.abs(xyz[:, :, 2]).unsqueeze(1)
    return torch.cat([xy, torch.abs(q[:, 2:])], 1).permute(0, 2, 1)


def world2cam(xyz, az, el, batch_size=None, device=None, N_PTS=1024):
    """projection.py:148-199: world -> camera co-ordinates for a camera at
    distance 2.5, azimuth az [B] and elevation el [B] (radians):
    R (p - t) with R = R_el R_az and t = (0, 0, -2.5).  Returns [B, N, 3] on
    xyz's device."""
    dev = xyz.device
    az = az.to(device=dev, dtype=xyz.dtype)
    el = el.to(device=dev, dtype=xyz.dtype)
    one, zero = torch.ones_like(az), torch.zeros_like(az)
    ca, sa, ce, se = torch.cos(az), torch.sin(az), torch.cos(el), torch.sin(el)
    r_az = torch.stack([torch.stack([one, zero, zero], 1),
                        torch.stack([zero, ca, -sa], 1),
                        torch.stack([zero, sa, ca], 1)], 1)  # [B, 3, 3]
    r_el = torch.stack([torch.stack([ce, zero, se], 1),
                        torch.stack([zero, one, zero], 1),
                        torch.stack([-se, zero, ce], 1)], 1)
    rot = torch.matmul(r_el, r_az)
    t = torch.tensor([0., 0., -2.5], dtype=xyz.dtype, device=dev)
    return torch.matmul(rot, (xyz - t).permute(0, 2, 1)).permute(0, 2, 1)
