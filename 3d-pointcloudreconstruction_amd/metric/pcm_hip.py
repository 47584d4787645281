"""ctypes binding of libpcm_hip.so (the gfx950 HIP kernels behind include/pcm.h).

This is the product path's only route to compute: there is no CPU fallback.
If the library is missing, or a tensor is not on a HIP device, every entry
point raises.  Kernels are enqueued on PyTorch's *current* stream of the
tensors' device (the reference launched on the legacy default stream,
chamfer3D.cu:142-143 -- SURVEY.md appendix A.5).
"""
from __future__ import annotations

import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get(
    "PCM_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libpcm_hip.so"))
# the tuning build (make -C csrc tune): the product library plus the measured
# alternatives of the one-launch Chamfer step (fused variants 0-19 beside the default 20), which
# tools/ and the variant tests select by number; never on the product path
TUNE_LIB_PATH = os.environ.get(
    "PCM_HIP_TUNE_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libpcm_hip_tune.so"))

_lib = None
_tune_lib = None

# every symbol include/pcm.h declares (checked by tests/test_capi.py)
EXPORTED = (
    "pcm_version", "pcm_strerror",
    "pcm_chamfer_forward", "pcm_chamfer_backward",
    "pcm_chamfer_workspace_bytes", "pcm_chamfer_forward_loss", "pcm_chamfer_workspace_status",
    "pcm_emd_workspace_bytes", "pcm_emd_forward", "pcm_emd_backward", "pcm_emd_workspace_status",
    "pcm_chamfer_forward_f16", "pcm_chamfer_backward_f16",
    "pcm_chamfer_forward_ws_bytes", "pcm_chamfer_forward_ws", "pcm_chamfer_forward_ws_f16",
    "pcm_chamfer_loss_grad", "pcm_chamfer_forward_layout", "pcm_chamfer_backward_layout",
    "pcm_chamfer_backward_strided", "pcm_chamfer_loss_grad_layout", "pcm_chamfer_loss_grad_rescale",
    "pcm_chamfer_loss_grad_steps",
    "pcm_chamfer_eval_workspace_bytes", "pcm_chamfer_eval", "pcm_chamfer_eval_f16",
    "pcm_chamfer_cross_workspace_bytes", "pcm_chamfer_cross",
    "pcm_chamfer_nd_forward", "pcm_chamfer_nd_backward",
    "pcm_silhouette_forward", "pcm_silhouette_backward", "pcm_proj_bce_workspace_bytes", "pcm_proj_bce",
    "pcm_fps",
    "pcm_knn", "pcm_repulsion_workspace_bytes", "pcm_repulsion_loss",
    "pcm_ball_query", "pcm_uniform_workspace_bytes", "pcm_uniform_loss",
    "pcm_kernel_loss_workspace_bytes", "pcm_kernel_loss",
    "pcm_sinkhorn_schedule", "pcm_sinkhorn_workspace_bytes", "pcm_sinkhorn_loss",
    "pcm_sliced_workspace_bytes", "pcm_sliced_wasserstein_loss",
    "pcm_dcd_workspace_bytes", "pcm_dcd_loss",
    "pcm_icp_workspace_bytes", "pcm_icp", "pcm_icp_workspace_status", "pcm_nearest_neighbor",
    "pcm_best_fit_transform",
    "pcm_npy_cloud_points", "pcm_npy_load_clouds",
)

# largest cloud pcm_icp takes (csrc/icp.hip kIcpMaxN: 16 slices of 1024 points)
ICP_MAX_POINTS = 16384

# largest cloud (points per batch element) pcm_chamfer_loss_grad runs as one
# launch (csrc/chamfer_filt.hip kGradCap); larger clouds take forward + backward
LOSS_GRAD_MAX_POINTS = 1024


class PcmError(RuntimeError):
    """A libpcm_hip call returned a non-zero pcm_status."""


def load_library():
    """Load libpcm_hip.so (raises OSError with the path if it is missing)."""
    global _lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


def load_tune_library():
    """Load libpcm_hip_tune.so, the tuning build (fused variants 0-19 beside
    the default); raises OSError if it is missing."""
    global _tune_lib
    if _tune_lib is None:
        _tune_lib = _open(TUNE_LIB_PATH)
    return _tune_lib


def _open(path):
    if not os.path.exists(path):
        raise OSError(
            f"{os.path.basename(path)} not found at {path}; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
            "3d-pointcloudreconstruction_amd/csrc`")
    L = ctypes.CDLL(path)
    vp, ci, cf, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    L.pcm_version.restype = ci
    L.pcm_version.argtypes = []
    L.pcm_strerror.restype = ctypes.c_char_p
    L.pcm_strerror.argtypes = [ci]
    L.pcm_chamfer_forward.restype = ci
    L.pcm_chamfer_forward.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.pcm_chamfer_backward.restype = ci
    L.pcm_chamfer_backward.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.pcm_chamfer_workspace_bytes.restype = cs
    L.pcm_chamfer_workspace_bytes.argtypes = [ci, ci, ci]
    L.pcm_chamfer_workspace_status.restype = ci
    L.pcm_chamfer_workspace_status.argtypes = [vp, cs, ci, ci, ci, vp]
    L.pcm_tune_chamfer_loss_grad_spins.restype = ci
    L.pcm_tune_chamfer_loss_grad_spins.argtypes = [ctypes.c_uint, ctypes.c_uint, vp, vp, ci, ci, ci, cf, cf, vp, vp,
                                                   vp, vp, vp, vp, vp, vp, cs, vp]
    L.pcm_tune_chamfer_slow_paths.restype = ci
    L.pcm_tune_chamfer_slow_paths.argtypes = [vp, cs, ci, ci, ci, vp]
    L.pcm_tune_chamfer_err_offset.restype = cs
    L.pcm_tune_chamfer_err_offset.argtypes = [ci, ci, ci, ci]
    L.pcm_chamfer_forward_loss.restype = ci
    L.pcm_chamfer_forward_loss.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, cs, vp]
    L.pcm_tune_num_chamfer_variants.restype = ci
    L.pcm_tune_num_chamfer_variants.argtypes = []
    L.pcm_tune_chamfer_forward.restype = ci
    L.pcm_tune_chamfer_forward.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.pcm_tune_chamfer_backward.restype = ci
    L.pcm_tune_chamfer_backward.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.pcm_tune_chamfer_forward_loss.restype = ci
    L.pcm_tune_chamfer_forward_loss.argtypes = [ci, ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_chamfer_forward_layout"):  # absent from A/B builds of older sources
        L.pcm_chamfer_forward_layout.restype = ci
        L.pcm_chamfer_forward_layout.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.pcm_chamfer_backward_layout.restype = ci
        L.pcm_chamfer_backward_layout.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "pcm_chamfer_backward_strided"):
        ll = ctypes.c_longlong
        L.pcm_chamfer_backward_strided.restype = ci
        L.pcm_chamfer_backward_strided.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ll, ll, vp, ll, ll, vp, vp, vp,
                                                   vp, vp]
    L.pcm_chamfer_forward_f16.restype = ci
    L.pcm_chamfer_forward_f16.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.pcm_chamfer_backward_f16.restype = ci
    L.pcm_chamfer_backward_f16.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "pcm_chamfer_forward_ws"):  # absent from A/B builds of older sources
        L.pcm_chamfer_forward_ws_bytes.restype = cs
        L.pcm_chamfer_forward_ws_bytes.argtypes = [ci, ci, ci]
        L.pcm_chamfer_forward_ws.restype = ci
        L.pcm_chamfer_forward_ws.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, cs, vp]
        L.pcm_chamfer_forward_ws_f16.restype = ci
        L.pcm_chamfer_forward_ws_f16.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, cs, vp]
        L.pcm_tune_chamfer_forward_grid_ws_bytes.restype = cs
        L.pcm_tune_chamfer_forward_grid_ws_bytes.argtypes = [ci, ci, ci]
        L.pcm_tune_chamfer_forward_grid.restype = ci
        L.pcm_tune_chamfer_forward_grid.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, cs, vp, vp]
        L.pcm_tune_chamfer_backward_f16.restype = ci
        L.pcm_tune_chamfer_backward_f16.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.pcm_tune_num_chamfer_f16_variants.restype = ci
    L.pcm_tune_num_chamfer_f16_variants.argtypes = []
    L.pcm_tune_chamfer_forward_f16.restype = ci
    L.pcm_tune_chamfer_forward_f16.argtypes = [ci, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp]
    L.pcm_emd_workspace_bytes.restype = cs
    L.pcm_emd_workspace_bytes.argtypes = [ci, ci]
    L.pcm_emd_forward.restype = ci
    L.pcm_emd_forward.argtypes = [vp, vp, ci, ci, cf, ci, vp, vp, vp, vp, cs, vp]
    L.pcm_emd_backward.restype = ci
    L.pcm_emd_backward.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
    L.pcm_emd_workspace_status.restype = ci
    L.pcm_emd_workspace_status.argtypes = [vp, cs, ci, ci, vp]
    L.pcm_tune_emd_forward_cfg.restype = ci
    L.pcm_tune_emd_forward_cfg.argtypes = [vp, vp, ci, ci, cf, ci, vp, vp, vp, vp, cs, ci, ci, ci, ci, ci, ci, vp,
                                           vp]
    L.pcm_tune_emd_timeouts.restype = ci
    L.pcm_tune_emd_timeouts.argtypes = [vp, cs, ci, ci, vp]
    L.pcm_chamfer_loss_grad.restype = ci
    L.pcm_chamfer_loss_grad.argtypes = [vp, vp, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp, cs, vp]
    L.pcm_tune_chamfer_loss_grad.restype = ci
    L.pcm_tune_chamfer_loss_grad.argtypes = [ci, vp, vp, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp, cs,
                                             vp]
    L.pcm_tune_num_chamfer_loss_grad_variants.restype = ci
    L.pcm_tune_num_chamfer_loss_grad_variants.argtypes = []
    if hasattr(L, "pcm_chamfer_loss_grad_layout"):  # absent from A/B builds of older sources
        L.pcm_chamfer_loss_grad_layout.restype = ci
        L.pcm_chamfer_loss_grad_layout.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp, vp,
                                                   vp, vp, cs, vp]
        L.pcm_chamfer_loss_grad_rescale.restype = ci
        L.pcm_chamfer_loss_grad_rescale.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp, vp,
                                                    vp]
        L.pcm_chamfer_loss_grad_steps.restype = ci
        L.pcm_chamfer_loss_grad_steps.argtypes = [ci, vp, vp, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  cs, vp]
    if hasattr(L, "pcm_chamfer_eval"):  # absent from A/B builds of older sources
        L.pcm_chamfer_eval_workspace_bytes.restype = cs
        L.pcm_chamfer_eval_workspace_bytes.argtypes = [ci, ci, ci, ci]
        for fn in (L.pcm_chamfer_eval, L.pcm_chamfer_eval_f16):
            fn.restype = ci
            fn.argtypes = [vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_silhouette_forward"):  # absent from A/B builds of older sources
        L.pcm_silhouette_forward.restype = ci
        L.pcm_silhouette_forward.argtypes = [vp, ci, ci, ci, ci, ci, cf, vp, vp]
        L.pcm_silhouette_backward.restype = ci
        L.pcm_silhouette_backward.argtypes = [vp, ci, ci, ci, ci, ci, cf, vp, vp, vp]
        L.pcm_proj_bce_workspace_bytes.restype = cs
        L.pcm_proj_bce_workspace_bytes.argtypes = [ctypes.c_longlong]
        L.pcm_proj_bce.restype = ci
        L.pcm_proj_bce.argtypes = [vp, vp, ctypes.c_longlong, cf, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_fps"):  # absent from A/B builds of older sources
        L.pcm_fps.restype = ci
        L.pcm_fps.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.pcm_tune_fps.restype = ci
        L.pcm_tune_fps.argtypes = [ci, vp, ci, ci, ci, ci, ci, vp, vp, vp]
        L.pcm_tune_fps_default_threads.restype = ci
        L.pcm_tune_fps_default_threads.argtypes = [ci]
    if hasattr(L, "pcm_knn"):  # absent from A/B builds of older sources
        L.pcm_knn.restype = ci
        L.pcm_knn.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
        L.pcm_tune_knn.restype = ci
        L.pcm_tune_knn.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
        L.pcm_tune_knn_default_split.restype = ci
        L.pcm_tune_knn_default_split.argtypes = [ci, ci]
        L.pcm_repulsion_workspace_bytes.restype = cs
        L.pcm_repulsion_workspace_bytes.argtypes = [ci, ci]
        L.pcm_repulsion_loss.restype = ci
        L.pcm_repulsion_loss.argtypes = [vp, ci, ci, ci, cf, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_ball_query"):  # absent from A/B builds of older sources
        L.pcm_ball_query.restype = ci
        L.pcm_ball_query.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, ci, vp, vp, vp]
        L.pcm_uniform_workspace_bytes.restype = cs
        L.pcm_uniform_workspace_bytes.argtypes = [ci, ci, ci, ci, vp]
        L.pcm_uniform_loss.restype = ci
        L.pcm_uniform_loss.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, vp, ctypes.c_double, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_kernel_loss"):  # absent from A/B builds of older sources
        L.pcm_kernel_loss_workspace_bytes.restype = cs
        L.pcm_kernel_loss_workspace_bytes.argtypes = [ci, ci, ci]
        L.pcm_kernel_loss.restype = ci
        L.pcm_kernel_loss.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_sinkhorn_loss"):  # absent from A/B builds of older sources
        L.pcm_sinkhorn_schedule.restype = ci
        L.pcm_sinkhorn_schedule.argtypes = [cf, cf, cf, vp, ci]
        L.pcm_sinkhorn_workspace_bytes.restype = cs
        L.pcm_sinkhorn_workspace_bytes.argtypes = [ci, ci, ci]
        L.pcm_sinkhorn_loss.restype = ci
        L.pcm_sinkhorn_loss.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_sliced_wasserstein_loss"):  # absent from A/B builds of older sources
        L.pcm_sliced_workspace_bytes.restype = cs
        L.pcm_sliced_workspace_bytes.argtypes = [ci, ci, ci, ci]
        L.pcm_sliced_wasserstein_loss.restype = ci
        L.pcm_sliced_wasserstein_loss.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, cs,
                                                  vp]
    if hasattr(L, "pcm_dcd_loss"):  # absent from A/B builds of older sources
        L.pcm_dcd_workspace_bytes.restype = cs
        L.pcm_dcd_workspace_bytes.argtypes = [ci, ci, ci]
        L.pcm_dcd_loss.restype = ci
        L.pcm_dcd_loss.argtypes = [vp, vp, ci, ci, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, cs, vp]
    if hasattr(L, "pcm_chamfer_cross"):  # absent from A/B builds of older sources
        L.pcm_chamfer_cross_workspace_bytes.restype = cs
        L.pcm_chamfer_cross_workspace_bytes.argtypes = [ci, ci, ci, ci]
        L.pcm_chamfer_cross.restype = ci
        L.pcm_chamfer_cross.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, cs, vp]
        L.pcm_tune_chamfer_cross_run.restype = ci
        L.pcm_tune_chamfer_cross_run.argtypes = [ci, ci, ci, ci, ci]
    if hasattr(L, "pcm_chamfer_nd_forward"):  # absent from A/B builds of older sources
        L.pcm_chamfer_nd_forward.restype = ci
        L.pcm_chamfer_nd_forward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.pcm_chamfer_nd_backward.restype = ci
        L.pcm_chamfer_nd_backward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.pcm_tune_chamfer_nd_geometry.restype = None
        L.pcm_tune_chamfer_nd_geometry.argtypes = [vp, vp, vp]
    if hasattr(L, "pcm_tune_occupy"):  # absent from A/B builds of older sources
        L.pcm_tune_occupy.restype = ci
        L.pcm_tune_occupy.argtypes = [ci, ci, ci, ctypes.c_uint, vp]
    if hasattr(L, "pcm_tune_occupy_stamped"):
        L.pcm_tune_occupy_stamped.restype = ci
        L.pcm_tune_occupy_stamped.argtypes = [ci, ci, ci, ctypes.c_uint, vp, vp]
        L.pcm_tune_clock_stamp.restype = ci
        L.pcm_tune_clock_stamp.argtypes = [vp, vp]
    if hasattr(L, "pcm_tune_clock_rate"):
        L.pcm_tune_clock_rate.restype = ci
        L.pcm_tune_clock_rate.argtypes = [vp, ci, vp]
    if hasattr(L, "pcm_tune_occupy_flagged"):
        L.pcm_tune_occupy_flagged.restype = ci
        L.pcm_tune_occupy_flagged.argtypes = [ci, ci, ci, ctypes.c_uint, vp, vp, vp]
    cd = ctypes.c_double
    L.pcm_icp.restype = ci
    L.pcm_icp.argtypes = [vp, vp, ci, ci, vp, ci, cd, vp, vp, vp, vp, cs, vp]
    L.pcm_icp_workspace_status.restype = ci
    L.pcm_icp_workspace_status.argtypes = [vp, cs, ci, ci, vp]
    L.pcm_icp_workspace_bytes.restype = cs
    L.pcm_icp_workspace_bytes.argtypes = [ci, ci]
    L.pcm_nearest_neighbor.restype = ci
    L.pcm_nearest_neighbor.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, cs, vp]
    L.pcm_best_fit_transform.restype = ci
    L.pcm_best_fit_transform.argtypes = [vp, vp, ci, ci, vp, vp]
    return L


def strerror(status: int) -> str:
    return load_library().pcm_strerror(int(status)).decode()


def _check(status: int, what: str) -> None:
    if status != 0:
        raise PcmError(f"{what} failed: {strerror(status)} (status {status})")


def _require_device(*tensors: torch.Tensor) -> torch.device:
    dev = tensors[0].device
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError(
                "pcm_hip kernels need HIP device tensors (got a tensor on "
                f"{t.device}); there is no CPU path")
        if t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _cloud_kind(xyz1, xyz2) -> str:
    if xyz1.dtype != xyz2.dtype or xyz1.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"Chamfer clouds must both be float32 or both float16 (got {xyz1.dtype}, {xyz2.dtype})")
    return "f16" if xyz1.dtype == torch.float16 else "f32"


# clouds at least this large (both) take the grid forward (csrc/chamfer_grid.hip
# kGridMinPoints), which needs pcm_chamfer_forward_ws_bytes of workspace
GRID_MIN_POINTS = 4096


def forward_workspace(dev: torch.device, b: int, n: int, m: int, force_grid: bool = False):
    """Scratch for the grid forward (no state between calls, no zero-fill):
    None when the problem takes the dense kernels (pcm_chamfer_forward_ws_bytes
    is 0), else ONE buffer per (device, current stream), grown when a larger
    problem needs more (it holds nothing between calls).  force_grid: the
    size the grid path needs at any problem size (tune_chamfer_forward_grid)."""
    L = load_library()
    need = int(L.pcm_tune_chamfer_forward_grid_ws_bytes(b, n, m) if force_grid
               else L.pcm_chamfer_forward_ws_bytes(b, n, m))
    if need == 0:
        return None
    key = ("forward", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def cloud_layout(t: torch.Tensor):
    """0 for a contiguous [B, N, 3] cloud (rows), 1 for a [B, N, 3] view of a
    contiguous [B, 3, N] tensor (channel planes: the generator output
    train.py:163 passes as fake.transpose(2, 1)), None for anything else."""
    if t.dim() != 3 or t.shape[2] != 3:
        return None
    b, n, _ = t.shape
    if t.is_contiguous():
        return 0
    st = t.stride()
    if (st[1] == 1 or n == 1) and st[2] == n and (st[0] == 3 * n or b == 1):
        return 1
    return None


def chamfer_forward_layout(xyz1, xyz2, lay1, lay2, dist1, dist2, idx1, idx2) -> None:
    """pcm_chamfer_forward_layout: float32 clouds each in rows (0) or channel
    planes (1, see cloud_layout); results identical to chamfer_forward on rows."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
        raise TypeError("chamfer_forward_layout takes float32 clouds")
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_forward_layout(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), _ptr(dist1), _ptr(dist2), _ptr(idx1),
            _ptr(idx2), _stream(dev)), "pcm_chamfer_forward_layout")


def chamfer_backward_layout(xyz1, xyz2, lay1, lay2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2) -> None:
    """pcm_chamfer_backward_layout: gradxyz1/2 written in their cloud's layout."""
    dev = _require_device(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_backward_layout(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), _ptr(graddist1), _ptr(graddist2), _ptr(idx1),
            _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2), _stream(dev)), "pcm_chamfer_backward_layout")


def chamfer_backward_strided(xyz1, xyz2, lay1, lay2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2) -> None:
    """pcm_chamfer_backward_strided: float32 [B, N] graddists read in place at
    their own strides (an expanded scalar included); gradients in their cloud's
    layout (lay 0 rows, 1 channel planes)."""
    dev = _require_device(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    for g, k in ((graddist1, n), (graddist2, m)):
        if g.dtype != torch.float32 or tuple(g.shape) != (b, k):
            raise ValueError("chamfer_backward_strided takes float32 graddists of shape [B, N] and [B, M]")
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_backward_strided(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), _ptr(graddist1), graddist1.stride(0),
            graddist1.stride(1), _ptr(graddist2), graddist2.stride(0), graddist2.stride(1), _ptr(idx1), _ptr(idx2),
            _ptr(gradxyz1), _ptr(gradxyz2), _stream(dev)), "pcm_chamfer_backward_strided")


def chamfer_forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> None:
    """pcm_chamfer_forward (float32 clouds) or pcm_chamfer_forward_f16 (float16
    clouds) on contiguous [B,N,3]/[B,M,3] device tensors; dist is float32.
    Clouds of >= GRID_MIN_POINTS points go through pcm_chamfer_forward_ws[_f16]
    (the grid forward; same outputs bit for bit)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    f16 = _cloud_kind(xyz1, xyz2) == "f16"
    L = load_library()
    with torch.cuda.device(dev):
        ws = forward_workspace(dev, b, n, m) if (n >= GRID_MIN_POINTS and m >= GRID_MIN_POINTS and b > 0) else None
        if ws is not None:  # the grid forward pays at this size (csrc/chamfer_grid.hip grid_pays)
            fn = "pcm_chamfer_forward_ws_f16" if f16 else "pcm_chamfer_forward_ws"
            _check(getattr(L, fn)(
                _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
                _ptr(ws), ws.numel(), _stream(dev)), fn)
            return
        fn = "pcm_chamfer_forward_f16" if f16 else "pcm_chamfer_forward"
        _check(getattr(L, fn)(
            _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
            _stream(dev)), fn)


def tune_chamfer_forward_grid(xyz1, xyz2, dist1, dist2, idx1, idx2, scan="filter", only=None,
                              stats=None, workspace=None, small_wg=False, reg_gather=False) -> None:
    """Internal: the grid forward at any size (float32 or float16 clouds).
    scan: "filter" (default: packed (u, w) screen + proof), "screened" (exact
    distances, chunk minima) or "exact" (every candidate's key); only =
    "build" / "search" runs one of its two kernels (search reuses the
    workspace of a previous call with the same clouds); stats: int32 device
    tensor, 12 ints per search wave (csrc/chamfer_grid.hip)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    f16 = _cloud_kind(xyz1, xyz2) == "f16"
    mode = int(f16) | {"filter": 0, "screened": 64, "exact": 2}[scan] | {None: 0, "build": 4, "search": 8}[only]
    mode |= (16 if small_wg else 0) | (32 if reg_gather else 0)
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else forward_workspace(dev, b, n, m, force_grid=True)
        _check(load_library().pcm_tune_chamfer_forward_grid(
            mode, _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
            _ptr(ws), ws.numel(), _stream(dev), _ptr(stats)), "pcm_tune_chamfer_forward_grid")


def tune_chamfer_forward_f16(variant, xyz1, xyz2, dist1, dist2, idx1, idx2) -> None:
    """Internal: fp16 forward variant `variant` (-1 = default)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_forward_f16(
            int(variant), _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1),
            _ptr(idx2), _stream(dev)), "pcm_tune_chamfer_forward_f16")


def tune_num_chamfer_f16_variants() -> int:
    return int(load_library().pcm_tune_num_chamfer_f16_variants())


# cached device workspaces: an LRU of at most _WS_CACHE_MAX buffers (the
# fused-loss workspaces are per shape; the grid forward's one per stream)
_ws_cache = collections.OrderedDict()
_WS_CACHE_MAX = 16
# every cached buffer handed out while a graph was being captured: the graph
# keeps its raw pointer, so the buffer must outlive any eviction or growth of
# the cache (else a replay would write into freed, possibly reused memory)
_graph_pinned = {}


def _cache_put(key, ws):
    _ws_cache[key] = ws
    _ws_cache.move_to_end(key)
    while len(_ws_cache) > _WS_CACHE_MAX:
        old_key, _ = _ws_cache.popitem(last=False)
        _watches.pop(old_key, None)


def _hand_out(ws):
    """A cached buffer about to be passed to a kernel: pinned for the life of
    the process if the current stream is capturing a graph."""
    if ws is not None and torch.cuda.is_current_stream_capturing():
        _graph_pinned.setdefault(ws.data_ptr(), ws)
    return ws


def _stream_id(dev: torch.device) -> int:
    return int(torch.cuda.current_stream(dev).cuda_stream)


def chamfer_workspace(dev: torch.device, b: int, n: int, m: int) -> torch.Tensor:
    """Zero-filled workspace for the fused-loss kernels, cached per (device,
    current stream, shape): the kernels keep cross-launch state in it (epoch,
    arrival counters, argmin granules), so only stream-ordered calls may share
    one; one per shape keeps every call's granules trusted (a workspace last
    used by another shape makes the next call recompute its argmins,
    csrc/chamfer_filt.hip kGradShapeWord)."""
    need = int(load_library().pcm_chamfer_workspace_bytes(b, n, m))
    if _tune_lib is not None:  # the tuning build's variants need more (all of them fit)
        need = max(need, int(_tune_lib.pcm_chamfer_workspace_bytes(b, n, m)))
    key = ("chamfer", dev, _stream_id(dev), b, n, m)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    else:
        _ws_cache.move_to_end(key)
    return _hand_out(ws)


_scale_hints = {}


def grad_scale_hint(dev: torch.device) -> torch.Tensor:
    """The upstream gradient the next one-launch Chamfer loss on (device,
    current stream) expects (a device float, 1.0 at first):
    chamfer_3DLossFunction's forward computes its gradient for this scale and
    its backward (pcm_chamfer_loss_grad_rescale) stores the real one here, so
    a training loop with a constant loss weight computes it right from its
    second step on.  Never freed (graphs keep its pointer)."""
    key = (dev, _stream_id(dev))
    t = _scale_hints.get(key)
    if t is None:
        last = _scale_hints.get(("last", dev))
        if last is not None and torch.cuda.is_current_stream_capturing():
            # a capture stream takes the device's last-used hint (the scale the
            # eager warm-up learned): a new tensor's fill would be captured and
            # reset the scale at every replay
            t = last
        else:
            t = torch.ones(1, dtype=torch.float32, device=dev)
        _scale_hints[key] = t
    _scale_hints[("last", dev)] = t
    return t


class _StickyWatch:
    """Lagged, sync-free check of a cached fused-loss workspace's sticky error
    words (a loss poll that timed out: NaN means from then on).  After every
    call the two words are copied asynchronously to pinned host memory behind
    an event, into a small ring of such copies; each call first reads the
    copies whose events have completed, oldest first, and, if a word is set,
    re-zeroes the workspace and raises PcmError, so a timeout is reported
    instead of silently persisting.  No copy is ever dropped: a host that
    runs ahead of the GPU fills the ring, and a full ring waits for its
    oldest copy, which bounds the calls between a timeout and its report.
    The words are copied after the first and then every `every`-th call (a copy is a
    kernel on the stream: two per call had cost ~9 us of GPU time per step
    of a ~17 us training call), so a timeout is reported within
    every * (depth + 1) calls; its NaN means are visible at once anyway."""

    depth = 4
    every = 32

    def __init__(self, ws, b, n, m):
        L = load_library()
        self.ws = ws
        self.offs = [int(L.pcm_tune_chamfer_err_offset(w, b, n, m)) for w in (0, 1)]
        self.bufs = [torch.zeros(2, dtype=torch.int32, pin_memory=True) for _ in range(self.depth)]
        self.ring = collections.deque()  # (buffer index, event), oldest first
        self.next = 0
        self.calls = 0

    def _read(self, k):
        if bool(self.bufs[k].any()):
            for kk, ev in self.ring:  # pending copies hold the same sticky words
                ev.synchronize()
            self.ring.clear()
            for buf in self.bufs:
                buf.zero_()
            self.ws.zero_()
            raise PcmError("a fused Chamfer loss kernel timed out waiting on its other workgroups "
                           "(NaN means); its workspace has been reset -- repeat the step")

    def check(self):
        while self.ring and self.ring[0][1].query():
            self._read(self.ring.popleft()[0])
        if len(self.ring) >= self.depth:
            k, ev = self.ring.popleft()
            ev.synchronize()
            self._read(k)

    def record(self):
        self.calls += 1
        if self.calls % self.every != 1 and self.every > 1:  # the first call, then every `every`-th
            return
        k = self.next
        self.next = (k + 1) % self.depth
        for i, o in enumerate(self.offs):
            self.bufs[k][i:i + 1].copy_(self.ws[o:o + 4].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.ring.append((k, ev))


_watches = {}


def _watched_workspace(dev, b, n, m):
    """The cached workspace plus its sticky-error watch (None under graph
    capture, where host reads and events are not part of the graph)."""
    ws = chamfer_workspace(dev, b, n, m)
    if torch.cuda.is_current_stream_capturing():
        return ws, None
    key = ("chamfer", dev, _stream_id(dev), b, n, m)
    w = _watches.get(key)
    if w is None or w.ws is not ws:
        w = _watches[key] = _StickyWatch(ws, b, n, m)
    w.check()
    return ws, w


def chamfer_forward_loss(xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out, workspace=None) -> None:
    """pcm_chamfer_forward_loss: forward + mean_out[0:2] = (mean(dist1), mean(dist2))."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    watch = None
    with torch.cuda.device(dev):
        if workspace is None:
            workspace, watch = _watched_workspace(dev, b, n, m)
        _check(load_library().pcm_chamfer_forward_loss(
            _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
            _ptr(mean_out), _ptr(workspace), workspace.numel(), _stream(dev)),
            "pcm_chamfer_forward_loss")
        if watch is not None:
            watch.record()


def loss_grad_supported(xyz1, xyz2) -> bool:
    """Whether pcm_chamfer_loss_grad takes these clouds in one launch."""
    return (xyz1.dtype == torch.float32 and xyz2.dtype == torch.float32 and xyz1.shape[0] > 0
            and 0 < xyz1.shape[1] <= LOSS_GRAD_MAX_POINTS and 0 < xyz2.shape[1] <= LOSS_GRAD_MAX_POINTS)


def chamfer_loss_grad(xyz1, xyz2, w1, w2, dist1, dist2, idx1, idx2, mean_out, gradxyz1, gradxyz2,
                      workspace=None, variant=None, layouts=(0, 0), grad_scale=None) -> None:
    """pcm_chamfer_loss_grad: the forward (dist/idx), mean_out[0:3] = (mean(dist1),
    mean(dist2), their sum), and the gradients of w1*sum(dist1) + w2*sum(dist2)
    w.r.t. both clouds, in one launch (float32, n, m <= LOSS_GRAD_MAX_POINTS).
    layouts / grad_scale: pcm_chamfer_loss_grad_layout (clouds and gradients
    in channel planes where layout is 1; the gradients for the expected
    upstream scale in the device float grad_scale, recorded in mean_out[3]).
    variant: a fused variant of the tuning build (libpcm_hip_tune.so)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    lay = (int(layouts[0]), int(layouts[1]))
    if mean_out.numel() < (3 if grad_scale is None else 4):
        raise ValueError("mean_out needs 3 floats (4 with grad_scale)")
    if variant is not None and (lay != (0, 0) or grad_scale is not None):
        raise ValueError("tuning variants take row clouds and no grad_scale")
    L = load_library() if variant is None else load_tune_library()
    watch = None
    with torch.cuda.device(dev):
        if workspace is None:
            workspace, watch = _watched_workspace(dev, b, n, m)
        tail = (_ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2), _ptr(mean_out), _ptr(gradxyz1), _ptr(gradxyz2),
                _ptr(workspace), workspace.numel(), _stream(dev))
        if variant is not None:
            _check(L.pcm_tune_chamfer_loss_grad(int(variant), _ptr(xyz1), _ptr(xyz2), b, n, m, float(w1), float(w2),
                                                *tail), "pcm_tune_chamfer_loss_grad")
        elif lay == (0, 0) and grad_scale is None:
            _check(L.pcm_chamfer_loss_grad(_ptr(xyz1), _ptr(xyz2), b, n, m, float(w1), float(w2), *tail),
                   "pcm_chamfer_loss_grad")
        else:
            if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.device != dev):
                raise ValueError("grad_scale must be a float32 tensor on the clouds' device")
            _check(L.pcm_chamfer_loss_grad_layout(_ptr(xyz1), _ptr(xyz2), b, n, m, lay[0], lay[1], float(w1),
                                                  float(w2), _ptr(grad_scale), *tail),
                   "pcm_chamfer_loss_grad_layout")
        if watch is not None:
            watch.record()


def chamfer_loss_grad_rescale(xyz1, xyz2, layouts, w1, w2, grad_loss, scale_used, scale_next, idx1, idx2,
                              gradxyz1, gradxyz2) -> None:
    """pcm_chamfer_loss_grad_rescale: the backward of a chamfer_loss_grad call
    made with grad_scale, now that the upstream gradient grad_loss (a device
    float) is known -- nothing when it equals scale_used bit for bit, else the
    exact gradients for it, in place; scale_next (nullable) receives it.
    scale_used None: always recompute."""
    dev = _require_device(xyz1, xyz2, grad_loss, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_loss_grad_rescale(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(layouts[0]), int(layouts[1]), float(w1), float(w2),
            _ptr(grad_loss), _ptr(scale_used), _ptr(scale_next), _ptr(idx1), _ptr(idx2), _ptr(gradxyz1),
            _ptr(gradxyz2), _stream(dev)), "pcm_chamfer_loss_grad_rescale")


def chamfer_workspace_status(workspace, b: int, n: int, m: int) -> None:
    """Raise PcmError if a fused-loss kernel on `workspace` hit a device-side
    timeout (sticky until the workspace is zero-filled again; synchronises the
    current stream)."""
    dev = workspace.device
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_workspace_status(_ptr(workspace), workspace.numel(), b, n, m, _stream(dev)),
               "pcm_chamfer_workspace_status")


def tune_chamfer_loss_grad_spins(wait_spins, poll_spins, xyz1, xyz2, w1, w2, dist1, dist2, idx1, idx2, mean_out,
                                 gradxyz1, gradxyz2, workspace) -> None:
    """Internal: pcm_chamfer_loss_grad with the gradient-phase waits bounded by
    wait_spins polls (0: every argmin recomputed locally -- exact results) and
    the loss poll by poll_spins (0 forces its timeout: sticky error, NaN means)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_loss_grad_spins(
            int(wait_spins), int(poll_spins), _ptr(xyz1), _ptr(xyz2), b, n, m, float(w1), float(w2), _ptr(dist1),
            _ptr(dist2), _ptr(idx1), _ptr(idx2), _ptr(mean_out), _ptr(gradxyz1), _ptr(gradxyz2), _ptr(workspace),
            workspace.numel(), _stream(dev)), "pcm_tune_chamfer_loss_grad_spins")


def chamfer_slow_paths(workspace, b: int, n: int, m: int) -> int:
    """Internal: gradient-phase waits on `workspace` that timed out and computed
    the missing argmins locally (since the workspace was zero-filled)."""
    dev = workspace.device
    with torch.cuda.device(dev):
        r = int(load_library().pcm_tune_chamfer_slow_paths(_ptr(workspace), workspace.numel(), b, n, m,
                                                           _stream(dev)))
    if r < 0:
        _check(r, "pcm_tune_chamfer_slow_paths")
    return r


def tune_occupy(dev: torch.device, blocks: int, threads: int, lds_bytes: int, usec: int, stamps=None,
                host_flag=None) -> None:
    """Internal (tests): hold `blocks` workgroups of `threads` threads and
    `lds_bytes` of LDS resident for `usec` microseconds on the current stream,
    issuing only s_sleep -- another kernel sharing the CUs.  stamps: an int64
    device tensor of 3, initialised to (-1, 0, 0): the earliest workgroup
    start, the latest end (s_memrealtime ticks, 100 MHz) and the count of
    workgroups that started.  host_flag: a pinned host int32 tensor the last
    workgroup to start sets to 1 (the host sees residency without a copy)."""
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_occupy_flagged(int(blocks), int(threads), int(lds_bytes), int(usec),
                                                      _ptr(stamps), _ptr(host_flag), _stream(dev)),
               "pcm_tune_occupy_flagged")


def tune_clock_stamp(out) -> None:
    """Internal (tests): a one-thread kernel on the current stream writes the
    GPU real-time clock (s_memrealtime, 100 MHz ticks) to the int64 device
    scalar `out`, or to pinned host memory (a store the host can poll; the
    current device's kernel)."""
    dev = out.device if out.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_clock_stamp(_ptr(out), _stream(dev)), "pcm_tune_clock_stamp")


def tune_clock_rate(out, iters: int = 20000) -> None:
    """Internal (tools/clock_state.py): one wave runs `iters` dependent FMAs on
    the current stream and writes (s_memrealtime ticks, s_memtime ticks) over
    them to out[0:2] (int64, device); the ratio x 0.1 is the shader clock in
    GHz while it ran."""
    with torch.cuda.device(out.device):
        _check(load_library().pcm_tune_clock_rate(_ptr(out), int(iters), _stream(out.device)), "pcm_tune_clock_rate")


def tune_num_chamfer_loss_grad_variants() -> int:
    """Fused variants of the tuning build (numbered 0 .. count - 1; the product
    library holds only the default, DEFAULT_LOSS_GRAD_VARIANT)."""
    return int(load_tune_library().pcm_tune_num_chamfer_loss_grad_variants())


# the product library's one-launch step (csrc/chamfer_filt.hip kDefaultGradVariant)
DEFAULT_LOSS_GRAD_VARIANT = 20


def mean_weight(count: int) -> float:
    """The per-element weight torch's mean backward multiplies the upstream
    gradient by: fl32(1 / count), as its device kernel forms it (a reciprocal
    then a multiply for a CPU-scalar divisor)."""
    import numpy as np
    return float(np.float32(1.0) / np.float32(count))


def tune_chamfer_forward(variant, xyz1, xyz2, dist1, dist2, idx1, idx2) -> None:
    """Internal: launch forward kernel variant `variant` (tools/tune_chamfer.py)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_forward(
            int(variant), _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2), _ptr(idx1),
            _ptr(idx2), _stream(dev)), "pcm_tune_chamfer_forward")


def tune_chamfer_backward_f16(variant, xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1,
                              gradxyz2) -> None:
    """Internal: fp16 backward `variant` (0 = automatic, 1 = 256-target workgroups, 3 = 1024-target)."""
    dev = _require_device(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_backward_f16(
            int(variant), _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(graddist1), _ptr(graddist2),
            _ptr(idx1), _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2), _stream(dev)),
            "pcm_tune_chamfer_backward_f16")


def tune_chamfer_backward(variant, xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1,
                          gradxyz2) -> None:
    """Internal: backward path `variant` (0 = automatic: staged, 1 = global-memory kernel, 2 = per-batch LDS
    kernel, 3 = global-memory kernel with 1024-target workgroups)."""
    dev = _require_device(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_backward(
            int(variant), _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(graddist1), _ptr(graddist2),
            _ptr(idx1), _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2), _stream(dev)),
            "pcm_tune_chamfer_backward")


def tune_chamfer_forward_loss(variant, loss_mode, xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out,
                              workspace=None) -> None:
    """Internal: fused-loss forward with an explicit variant (-1 = default) and
    loss mode (1 = in-kernel ticket, 2 = partials + finalize kernel)."""
    dev = _require_device(xyz1, xyz2, dist1, dist2, idx1, idx2, mean_out)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if workspace is None:
        workspace = chamfer_workspace(dev, b, n, m)
    with torch.cuda.device(dev):
        _check(load_library().pcm_tune_chamfer_forward_loss(
            int(variant), int(loss_mode), _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(dist1), _ptr(dist2),
            _ptr(idx1), _ptr(idx2), _ptr(mean_out), _ptr(workspace), workspace.numel(), _stream(dev)),
            "pcm_tune_chamfer_forward_loss")


def tune_num_chamfer_variants() -> int:
    return int(load_library().pcm_tune_num_chamfer_variants())


def chamfer_backward(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2) -> None:
    """pcm_chamfer_backward (float32 clouds and gradients) or pcm_chamfer_backward_f16
    (float16 clouds and gradients); graddist is float32 in both."""
    dev = _require_device(xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    kind = _cloud_kind(xyz1, xyz2)
    if gradxyz1.dtype != xyz1.dtype or gradxyz2.dtype != xyz2.dtype:
        raise TypeError("gradients must have the clouds' dtype")
    fn = "pcm_chamfer_backward_f16" if kind == "f16" else "pcm_chamfer_backward"
    with torch.cuda.device(dev):
        _check(getattr(load_library(), fn)(
            _ptr(xyz1), _ptr(xyz2), b, n, m, _ptr(graddist1), _ptr(graddist2), _ptr(idx1),
            _ptr(idx2), _ptr(gradxyz1), _ptr(gradxyz2), _stream(dev)), fn)


EVAL_MAX_THRESHOLDS = 8  # csrc/chamfer_eval.hip kEvalMaxTh


def chamfer_eval_workspace(dev: torch.device, b: int, n: int, m: int, nth: int) -> torch.Tensor:
    """Scratch for chamfer_eval (the workgroups' partial records): ONE buffer
    per (device, current stream), grown when a larger problem needs more; its
    content on entry is irrelevant and it holds nothing between calls."""
    need = max(int(load_library().pcm_chamfer_eval_workspace_bytes(b, n, m, nth)), 1)
    key = ("eval", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def chamfer_eval(xyz1, xyz2, thresholds, mean_dist, counts, scores, batch_scores=None, workspace=None) -> None:
    """pcm_chamfer_eval (float32 clouds) or pcm_chamfer_eval_f16 (float16) on
    contiguous [B,N,3]/[B,M,3] device tensors: for the 1..8 squared-distance
    `thresholds` (host floats) mean_dist [B,2] float32, counts [B,T,2] int32,
    scores [B,T,3] float32 = (F-score, p_x, p_y) and, when given, batch_scores
    [T,3] float32 (include/pcm.h).  Two launches; no per-point output."""
    tensors = (xyz1, xyz2, mean_dist, counts, scores) + (() if batch_scores is None else (batch_scores,))
    dev = _require_device(*tensors)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    th = [float(t) for t in thresholds]
    nth = len(th)
    if not 1 <= nth <= EVAL_MAX_THRESHOLDS:
        raise ValueError(f"chamfer_eval takes 1..{EVAL_MAX_THRESHOLDS} thresholds (got {nth})")
    f16 = _cloud_kind(xyz1, xyz2) == "f16"
    if xyz2.shape[0] != b or xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        raise ValueError("chamfer_eval takes clouds [B, N, 3] and [B, M, 3]")
    if not (xyz1.is_contiguous() and xyz2.is_contiguous()):
        raise ValueError("chamfer_eval takes contiguous clouds")
    for t, shape, dtype in ((mean_dist, (b, 2), torch.float32), (counts, (b, nth, 2), torch.int32),
                            (scores, (b, nth, 3), torch.float32)) + (
                                () if batch_scores is None else ((batch_scores, (nth, 3), torch.float32),)):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"chamfer_eval output must be contiguous {dtype} of shape {shape}")
    th_arr = (ctypes.c_float * nth)(*th)
    fn = "pcm_chamfer_eval_f16" if f16 else "pcm_chamfer_eval"
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = chamfer_eval_workspace(dev, b, n, m, nth)
        _check(getattr(load_library(), fn)(
            _ptr(xyz1), _ptr(xyz2), b, n, m, th_arr, nth, _ptr(mean_dist), _ptr(counts), _ptr(scores),
            _ptr(batch_scores), _ptr(workspace), workspace.numel(), _stream(dev)), fn)


SILHOUETTE_MAX_GRID = 128  # include/pcm.h PCM_SILHOUETTE_MAX_GRID


def _silhouette_args(xyz, layout, grid_h, grid_w, sigma_sq):
    if xyz.dtype != torch.float32:
        raise TypeError(f"the silhouette kernels take float32 clouds (got {xyz.dtype})")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("the silhouette kernels take clouds [B, N, 3]")
    if cloud_layout(xyz) != int(layout):
        raise ValueError("the cloud is not in the layout given (pcm_hip.cloud_layout)")
    return xyz.shape[0], xyz.shape[1], int(layout), int(grid_h), int(grid_w), float(sigma_sq)


def silhouette_forward(xyz, layout, grid_h, grid_w, sigma_sq, sil) -> None:
    """pcm_silhouette_forward: sil [B, grid_h, grid_w] float32 (contiguous) =
    the Gaussian-splatted silhouette of the float32 cloud xyz [B, N, 3], given
    as rows (layout 0) or as a view of channel planes (1, see cloud_layout)."""
    dev = _require_device(xyz, sil)
    b, n, lay, gh, gw, s2 = _silhouette_args(xyz, layout, grid_h, grid_w, sigma_sq)
    if tuple(sil.shape) != (b, gh, gw) or sil.dtype != torch.float32 or not sil.is_contiguous():
        raise ValueError(f"sil must be contiguous float32 of shape {(b, gh, gw)}")
    with torch.cuda.device(dev):
        _check(load_library().pcm_silhouette_forward(_ptr(xyz), b, n, lay, gh, gw, s2, _ptr(sil), _stream(dev)),
               "pcm_silhouette_forward")


def silhouette_backward(xyz, layout, grid_h, grid_w, sigma_sq, grad_sil, gradxyz) -> None:
    """pcm_silhouette_backward: gradxyz (xyz's shape and layout) from grad_sil
    [B, grid_h, grid_w] float32 (contiguous); gradxyz[..., 2] = 0."""
    dev = _require_device(xyz, grad_sil, gradxyz)
    b, n, lay, gh, gw, s2 = _silhouette_args(xyz, layout, grid_h, grid_w, sigma_sq)
    if tuple(grad_sil.shape) != (b, gh, gw) or grad_sil.dtype != torch.float32 or not grad_sil.is_contiguous():
        raise ValueError(f"grad_sil must be contiguous float32 of shape {(b, gh, gw)}")
    if gradxyz.dtype != torch.float32 or gradxyz.shape != xyz.shape or cloud_layout(gradxyz) != lay:
        raise ValueError("gradxyz must have the cloud's dtype, shape and layout")
    with torch.cuda.device(dev):
        _check(load_library().pcm_silhouette_backward(_ptr(xyz), b, n, lay, gh, gw, s2, _ptr(grad_sil),
                                                      _ptr(gradxyz), _stream(dev)), "pcm_silhouette_backward")


def proj_bce_workspace(dev: torch.device, count: int) -> torch.Tensor:
    """Scratch for proj_bce (the workgroups' partial sums): ONE buffer per
    (device, current stream), grown when a larger problem needs more; its
    content on entry is irrelevant and it holds nothing between calls."""
    need = max(int(load_library().pcm_proj_bce_workspace_bytes(count)), 1)
    key = ("bce", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def proj_bce(pred, gt, w, loss_out, grad_pred=None, workspace=None) -> None:
    """pcm_proj_bce on contiguous float32 device tensors pred, gt of one shape:
    loss_out[0] = the mean 'bce_prob' term (loss/proj_loss.py:17-19, :43) and,
    when given, grad_pred = its gradient with respect to pred."""
    tensors = (pred, gt, loss_out) + (() if grad_pred is None else (grad_pred,))
    dev = _require_device(*tensors)
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("proj_bce takes contiguous float32 tensors")
    if pred.shape != gt.shape or (grad_pred is not None and grad_pred.shape != pred.shape):
        raise ValueError("proj_bce takes pred, gt and grad_pred of one shape")
    if loss_out.numel() < 1:
        raise ValueError("loss_out needs one float")
    count = pred.numel()
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = proj_bce_workspace(dev, count)
        _check(load_library().pcm_proj_bce(_ptr(pred), _ptr(gt), count, float(w), _ptr(loss_out), _ptr(grad_pred),
                                           _ptr(workspace), workspace.numel(), _stream(dev)), "pcm_proj_bce")


FPS_MAX_POINTS = 16384  # include/pcm.h PCM_FPS_MAX_POINTS
FPS_THREADS = (64, 256, 1024)  # workgroup sizes of csrc/sampling.hip


def fps_default_threads(n: int) -> int:
    """The workgroup size pcm_fps picks for clouds of n points (csrc/sampling.hip)."""
    return int(load_library().pcm_tune_fps_default_threads(int(n)))


def fps(xyz, layout, npoint, start, idx_out, sampled_out=None, threads=None) -> None:
    """pcm_fps: idx_out [B, npoint] int64 (contiguous) = the farthest point
    samples of the float32 cloud xyz [B, N, 3], given as rows (layout 0) or as
    a view of channel planes (1, see cloud_layout), every cloud starting at
    index `start`; sampled_out (optional, contiguous float32 [B, npoint, 3])
    receives the sampled points from the same launch.  threads: internal
    (tests, tools/bench_fps.py) -- force the workgroup size, one of FPS_THREADS."""
    tensors = (xyz, idx_out) + (() if sampled_out is None else (sampled_out,))
    dev = _require_device(*tensors)
    if xyz.dtype != torch.float32:
        raise TypeError(f"fps takes float32 clouds (got {xyz.dtype})")
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError("fps takes clouds [B, N, 3]")
    if cloud_layout(xyz) != int(layout):
        raise ValueError("the cloud is not in the layout given (pcm_hip.cloud_layout)")
    b, n = xyz.shape[0], xyz.shape[1]
    npoint, start = int(npoint), int(start)
    if tuple(idx_out.shape) != (b, npoint) or idx_out.dtype != torch.int64 or not idx_out.is_contiguous():
        raise ValueError(f"idx_out must be contiguous int64 of shape {(b, npoint)}")
    if sampled_out is not None and (tuple(sampled_out.shape) != (b, npoint, 3) or sampled_out.dtype != torch.float32
                                    or not sampled_out.is_contiguous()):
        raise ValueError(f"sampled_out must be contiguous float32 of shape {(b, npoint, 3)}")
    with torch.cuda.device(dev):
        tail = (_ptr(xyz), b, n, int(layout), npoint, start, _ptr(idx_out), _ptr(sampled_out), _stream(dev))
        if threads is None:
            _check(load_library().pcm_fps(*tail), "pcm_fps")
        else:
            _check(load_library().pcm_tune_fps(int(threads), *tail), "pcm_tune_fps")


KNN_MAX_K = 32  # include/pcm.h PCM_KNN_MAX_K
KNN_MAX_POINTS = 16384  # include/pcm.h PCM_KNN_MAX_POINTS
KNN_WIDTHS = (4, 8, 16, 20, 32)  # list widths of csrc/knn.hip: k takes the first at or above it
KNN_TILE = 1024  # reference points per LDS tile of csrc/knn.hip (kKnnTile)
KNN_QUERIES = 64  # queries per workgroup of csrc/knn.hip
KNN_SPLIT = 4  # waves the reference cloud is split over when the grid is small (kKnnSplit)
KNN_VARIANTS = (0, 1, 2, 3)  # pcm_tune_knn: default, insert at once (libpcm_hip_tune.so), queued one wave, queued KNN_SPLIT waves
REPULSION_K = 5  # slot 0 and the four slots pcm_repulsion_loss reads
REPULSION_POINTS = 64  # points per workgroup of the repulsion kernel (kRepPoints)


def knn_default_split(b: int, n: int) -> int:
    """Waves per 64 queries pcm_knn picks for b clouds of n queries (csrc/knn.hip): KNN_SPLIT or 1."""
    return int(load_library().pcm_tune_knn_default_split(int(b), int(n)))


def _knn_cloud(t, layout, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what} takes float32 clouds (got {t.dtype})")
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{what} takes clouds [B, N, 3]")
    if cloud_layout(t) != int(layout):
        raise ValueError("the cloud is not in the layout given (pcm_hip.cloud_layout)")


def knn(query, lay_q, ref, lay_r, k, dist, idx, variant=None) -> None:
    """pcm_knn: dist [B, N, k] float32 (squared) and idx [B, N, k] int32, both
    contiguous = for every point of the float32 cloud query [B, N, 3] its k
    nearest points of ref [B, M, 3] in ascending (distance, index) order, empty
    slots (+inf, -1); each cloud given as rows (layout 0) or as a view of
    channel planes (1, see cloud_layout).  variant: internal (tests,
    tools/bench_knn.py) -- force a kernel form, one of KNN_VARIANTS (pcm_tune_knn)."""
    dev = _require_device(query, ref, dist, idx)
    _knn_cloud(query, lay_q, "knn")
    _knn_cloud(ref, lay_r, "knn")
    b, n, m, k = query.shape[0], query.shape[1], ref.shape[1], int(k)
    if ref.shape[0] != b:
        raise ValueError("knn takes clouds of one batch size")
    for t, dtype in ((dist, torch.float32), (idx, torch.int32)):
        if tuple(t.shape) != (b, n, k) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"knn output must be contiguous {dtype} of shape {(b, n, k)}")
    with torch.cuda.device(dev):
        tail = (_ptr(query), _ptr(ref), b, n, m, int(lay_q), int(lay_r), k, _ptr(dist), _ptr(idx), _stream(dev))
        if variant is None:
            _check(load_library().pcm_knn(*tail), "pcm_knn")
        else:  # the insert-at-once form is compiled into the tuning build only
            L = load_tune_library() if int(variant) == 1 else load_library()
            _check(L.pcm_tune_knn(int(variant), *tail), "pcm_tune_knn")


def repulsion_workspace(dev: torch.device, b: int, n: int) -> torch.Tensor:
    """Scratch for repulsion_loss (the k = 5 lists and the workgroups' partial
    sums): ONE buffer per (device, current stream), grown when a larger problem
    needs more; its content on entry is irrelevant and it holds nothing between calls."""
    need = max(int(load_library().pcm_repulsion_workspace_bytes(b, n)), 8)
    key = ("repulsion", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def repulsion_loss(xyz, lay, h, loss_out, gradxyz=None, workspace=None) -> None:
    """pcm_repulsion_loss: loss_out[0] = mean over the points of the float32
    cloud xyz [B, N, 3] (rows, or a view of channel planes: lay 1) and their
    nearest four other list slots of max(0, h - squared distance) and, when
    given, gradxyz (xyz's shape and layout) = its full gradient."""
    tensors = (xyz, loss_out) + (() if gradxyz is None else (gradxyz,))
    dev = _require_device(*tensors)
    _knn_cloud(xyz, lay, "repulsion_loss")
    if loss_out.dtype != torch.float32 or loss_out.numel() < 1:
        raise ValueError("loss_out needs one float32")
    if gradxyz is not None and (gradxyz.dtype != torch.float32 or gradxyz.shape != xyz.shape
                                or cloud_layout(gradxyz) != int(lay)):
        raise ValueError("gradxyz must have the cloud's dtype, shape and layout")
    b, n = xyz.shape[0], xyz.shape[1]
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = repulsion_workspace(dev, b, n)
        _check(load_library().pcm_repulsion_loss(_ptr(xyz), b, n, int(lay), float(h), _ptr(loss_out), _ptr(gradxyz),
                                                 _ptr(workspace), workspace.numel(), _stream(dev)),
               "pcm_repulsion_loss")


BALL_MAX_NSAMPLE = 64  # include/pcm.h PCM_BALL_MAX_NSAMPLE
UNIFORM_MAX_SCALES = 8  # include/pcm.h PCM_UNIFORM_MAX_SCALES
BALL_TILE = 1024  # cloud points per LDS tile of csrc/grouping.hip (kBallTile)
BALL_CENTRES = 4  # centres (waves) per workgroup of csrc/grouping.hip (kBallWaves)


def ball_query(xyz, lay_x, new_xyz, lay_c, radius, nsample, idx, cnt=None) -> None:
    """pcm_ball_query: idx [B, S, nsample] int32 (contiguous) = for every centre
    of new_xyz [B, S, 3] the first nsample points of the float32 cloud xyz
    [B, N, 3], in index order, whose pinned squared distance is below
    fl(radius * radius), padded with the first hit (all 0 without one); cnt
    (optional, [B, S] int32) = min(hits, nsample).  Each cloud is given as rows
    (layout 0) or as a view of channel planes (1, see cloud_layout)."""
    tensors = (xyz, new_xyz, idx) + (() if cnt is None else (cnt,))
    dev = _require_device(*tensors)
    _knn_cloud(xyz, lay_x, "ball_query")
    _knn_cloud(new_xyz, lay_c, "ball_query")
    b, n, s, nsample = xyz.shape[0], xyz.shape[1], new_xyz.shape[1], int(nsample)
    if new_xyz.shape[0] != b:
        raise ValueError("ball_query takes clouds of one batch size")
    if tuple(idx.shape) != (b, s, nsample) or idx.dtype != torch.int32 or not idx.is_contiguous():
        raise ValueError(f"ball_query idx must be contiguous int32 of shape {(b, s, nsample)}")
    if cnt is not None and (tuple(cnt.shape) != (b, s) or cnt.dtype != torch.int32 or not cnt.is_contiguous()):
        raise ValueError(f"ball_query cnt must be contiguous int32 of shape {(b, s)}")
    with torch.cuda.device(dev):
        _check(load_library().pcm_ball_query(_ptr(xyz), _ptr(new_xyz), b, n, s, int(lay_x), int(lay_c), float(radius),
                                             nsample, _ptr(idx), _ptr(cnt), _stream(dev)), "pcm_ball_query")


def _int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def uniform_workspace(dev: torch.device, b: int, n: int, npoint: int, nsample) -> torch.Tensor:
    """Scratch for uniform_loss (the seeds and one record per group slot): ONE
    buffer per (device, current stream), grown when a larger problem needs more;
    its content on entry is irrelevant and it holds nothing between calls."""
    need = max(int(load_library().pcm_uniform_workspace_bytes(b, n, int(npoint), len(nsample), _int_array(nsample))),
               8)
    key = ("uniform", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def uniform_loss(xyz, lay, npoint, nsample, ball_radius, weight, expect_len, loss_out, gradxyz=None, groups=None,
                 workspace=None) -> None:
    """pcm_uniform_loss on the float32 cloud xyz [B, N, 3] (rows, or a view of
    channel planes: lay 1): loss_out[0] = the uniform loss over npoint farthest
    point seeds and the scales (nsample[q], ball_radius[q], weight[q]) -- host
    sequences of one length -- around expect_len; when given, gradxyz (xyz's
    shape and layout) = its full gradient and groups ([B, npoint, sum nsample]
    int32, contiguous) = the seeds' index lists, scale after scale."""
    tensors = (xyz, loss_out) + tuple(t for t in (gradxyz, groups) if t is not None)
    dev = _require_device(*tensors)
    _knn_cloud(xyz, lay, "uniform_loss")
    if loss_out.dtype != torch.float32 or loss_out.numel() < 1:
        raise ValueError("loss_out needs one float32")
    if gradxyz is not None and (gradxyz.dtype != torch.float32 or gradxyz.shape != xyz.shape
                                or cloud_layout(gradxyz) != int(lay)):
        raise ValueError("gradxyz must have the cloud's dtype, shape and layout")
    nsample = [int(v) for v in nsample]
    if not (len(nsample) == len(ball_radius) == len(weight)):
        raise ValueError("uniform_loss takes nsample, ball_radius and weight of one length")
    b, n, npoint = xyz.shape[0], xyz.shape[1], int(npoint)
    if groups is not None and (tuple(groups.shape) != (b, npoint, sum(nsample)) or groups.dtype != torch.int32
                               or not groups.is_contiguous()):
        raise ValueError(f"groups must be contiguous int32 of shape {(b, npoint, sum(nsample))}")
    radii = (ctypes.c_float * len(nsample))(*[float(v) for v in ball_radius])
    weights = (ctypes.c_double * len(nsample))(*[float(v) for v in weight])
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = uniform_workspace(dev, b, n, npoint, nsample)
        _check(load_library().pcm_uniform_loss(_ptr(xyz), b, n, int(lay), npoint, len(nsample), _int_array(nsample),
                                               radii, weights, float(expect_len), _ptr(loss_out), _ptr(gradxyz),
                                               _ptr(groups), _ptr(workspace), workspace.numel(), _stream(dev)),
               "pcm_uniform_loss")


KERNEL_GAUSSIAN, KERNEL_LAPLACIAN, KERNEL_ENERGY = 0, 1, 2  # include/pcm.h PCM_KERNEL_*
KERNEL_LOSS_MAX_POINTS = 16384  # include/pcm.h PCM_KERNEL_LOSS_MAX_POINTS
KERNEL_LOSS_ROWS = 128  # row points per workgroup of csrc/kernel_loss.hip (kKlRows: two to a lane)
KERNEL_LOSS_TILE = 1024  # column points per LDS tile of csrc/kernel_loss.hip (kKlTile), an eighth to a wave
KERNEL_LOSS_WAVES = 8  # waves that share a tile (kKlWaves)


def kernel_loss_chain(n: int, m: int) -> int:
    """The longest chain of float32 additions behind a row sum of
    pcm_kernel_loss (include/pcm.h): wave 0's share of the larger cloud plus
    the additions that merge the waves."""
    share = KERNEL_LOSS_TILE // KERNEL_LOSS_WAVES
    return max(share * (c // KERNEL_LOSS_TILE) + min(share, c % KERNEL_LOSS_TILE) + KERNEL_LOSS_WAVES - 1
               for c in (int(n), int(m)))


def kernel_loss_workspace(dev: torch.device, b: int, n: int, m: int) -> torch.Tensor:
    """Scratch for kernel_loss (two float32 sums per point): ONE buffer per
    (device, current stream), grown when a larger problem needs more; its
    content on entry is irrelevant and it holds nothing between calls."""
    need = max(int(load_library().pcm_kernel_loss_workspace_bytes(b, n, m)), 8)
    key = ("kernel_loss", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def kernel_loss(xyz1, lay1, xyz2, lay2, kernel, blur, loss_out, gradxyz1=None, gradxyz2=None, workspace=None) -> None:
    """pcm_kernel_loss on the float32 clouds xyz1 [B, N, 3] and xyz2 [B, M, 3]
    (each rows, or a view of channel planes: layout 1): loss_out [B] = the
    kernel norm 1/2 |alpha - beta|^2_k of the two uniformly weighted clouds of
    every element for kernel KERNEL_GAUSSIAN / _LAPLACIAN / _ENERGY at `blur`;
    gradxyz1 / gradxyz2 (each optional; its cloud's shape and layout) = the
    gradient of loss_out[bi] in that cloud."""
    tensors = (xyz1, xyz2, loss_out) + tuple(t for t in (gradxyz1, gradxyz2) if t is not None)
    dev = _require_device(*tensors)
    _knn_cloud(xyz1, lay1, "kernel_loss")
    _knn_cloud(xyz2, lay2, "kernel_loss")
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if xyz2.shape[0] != b:
        raise ValueError("kernel_loss takes clouds of one batch size")
    if loss_out.dtype != torch.float32 or tuple(loss_out.shape) != (b,) or not loss_out.is_contiguous():
        raise ValueError(f"loss_out must be contiguous float32 of shape {(b,)}")
    for g, x, lay in ((gradxyz1, xyz1, lay1), (gradxyz2, xyz2, lay2)):
        if g is not None and (g.dtype != torch.float32 or g.shape != x.shape or cloud_layout(g) != int(lay)):
            raise ValueError("a gradient must have its cloud's dtype, shape and layout")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = kernel_loss_workspace(dev, b, n, m)
        _check(load_library().pcm_kernel_loss(_ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), int(kernel),
                                              float(blur), _ptr(loss_out), _ptr(gradxyz1), _ptr(gradxyz2),
                                              _ptr(workspace), workspace.numel(), _stream(dev)), "pcm_kernel_loss")


SINKHORN_MAX_POINTS = 16384  # include/pcm.h PCM_SINKHORN_MAX_POINTS
SINKHORN_MAX_STEPS = 128  # include/pcm.h PCM_SINKHORN_MAX_STEPS


def sinkhorn_schedule(blur: float, scaling: float, diameter: float) -> list:
    """pcm_sinkhorn_schedule: the epsilon list of pcm_sinkhorn_loss for
    (blur, scaling, diameter) as Python floats -- diameter^2 twice, then down
    by scaling^2 an entry while above blur^2, then blur^2.  Host only."""
    eps = (ctypes.c_double * SINKHORN_MAX_STEPS)()
    count = int(load_library().pcm_sinkhorn_schedule(float(blur), float(scaling), float(diameter), eps,
                                                     SINKHORN_MAX_STEPS))
    _check(min(count, 0), "pcm_sinkhorn_schedule")
    return [float(eps[k]) for k in range(count)]


def sinkhorn_workspace(dev: torch.device, b: int, n: int, m: int) -> torch.Tensor:
    """Scratch for sinkhorn_loss (two halves of two float32 potentials per
    point): ONE buffer per (device, current stream), grown when a larger
    problem needs more; its content on entry is irrelevant and it holds nothing
    between calls."""
    need = max(int(load_library().pcm_sinkhorn_workspace_bytes(b, n, m)), 8)
    key = ("sinkhorn", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def sinkhorn_loss(xyz1, lay1, xyz2, lay2, blur, scaling, diameter, loss_out, gradxyz1=None, gradxyz2=None,
                  potentials=None, workspace=None) -> None:
    """pcm_sinkhorn_loss on the float32 clouds xyz1 [B, N, 3] and xyz2
    [B, M, 3] (each rows, or a view of channel planes: layout 1): loss_out [B]
    = the debiased Sinkhorn divergence (p = 2, uniform weights) of every
    element at `blur`, reached by epsilon-scaling with ratio `scaling` from
    `diameter` (a host number: an upper bound of the clouds' extent);
    gradxyz1 / gradxyz2 (each optional; its cloud's shape and layout) = the
    gradient of loss_out[bi] in that cloud; potentials (optional, contiguous
    [B, N + M, 2]) = the last step's (F_cross, F_own) of every point."""
    tensors = (xyz1, xyz2, loss_out) + tuple(t for t in (gradxyz1, gradxyz2, potentials) if t is not None)
    dev = _require_device(*tensors)
    _knn_cloud(xyz1, lay1, "sinkhorn_loss")
    _knn_cloud(xyz2, lay2, "sinkhorn_loss")
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if xyz2.shape[0] != b:
        raise ValueError("sinkhorn_loss takes clouds of one batch size")
    if loss_out.dtype != torch.float32 or tuple(loss_out.shape) != (b,) or not loss_out.is_contiguous():
        raise ValueError(f"loss_out must be contiguous float32 of shape {(b,)}")
    for g, x, lay in ((gradxyz1, xyz1, lay1), (gradxyz2, xyz2, lay2)):
        if g is not None and (g.dtype != torch.float32 or g.shape != x.shape or cloud_layout(g) != int(lay)):
            raise ValueError("a gradient must have its cloud's dtype, shape and layout")
    if potentials is not None and (potentials.dtype != torch.float32 or tuple(potentials.shape) != (b, n + m, 2)
                                   or not potentials.is_contiguous()):
        raise ValueError(f"potentials must be contiguous float32 of shape {(b, n + m, 2)}")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = sinkhorn_workspace(dev, b, n, m)
        _check(load_library().pcm_sinkhorn_loss(_ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), float(blur),
                                                float(scaling), float(diameter), _ptr(loss_out), _ptr(gradxyz1),
                                                _ptr(gradxyz2), _ptr(potentials), _ptr(workspace),
                                                workspace.numel(), _stream(dev)), "pcm_sinkhorn_loss")


SLICED_MAX_POINTS = 16384  # include/pcm.h PCM_SLICED_MAX_POINTS
SLICED_MAX_DIRS = 1024  # include/pcm.h PCM_SLICED_MAX_DIRS
SLICED_FUSED_MAX_POINTS = 2048  # include/pcm.h PCM_SLICED_FUSED_MAX_POINTS


def sliced_workspace_bytes(b: int, n: int, m: int, l: int) -> int:
    return int(load_library().pcm_sliced_workspace_bytes(int(b), int(n), int(m), int(l)))


def sliced_workspace(dev: torch.device, b: int, n: int, m: int, l: int) -> torch.Tensor:
    """Scratch for sliced_wasserstein_loss (the slices, the points'
    coefficients and, for large clouds, the sorted lists): ONE buffer per
    (device, current stream), grown when a larger problem needs more; its
    content on entry is irrelevant and it holds nothing between calls."""
    need = max(sliced_workspace_bytes(b, n, m, l), 8)
    key = ("sliced", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def sliced_wasserstein_loss(xyz1, lay1, xyz2, lay2, dirs, loss_out, slices=None, gradxyz1=None, gradxyz2=None,
                            order1=None, order2=None, workspace=None) -> None:
    """pcm_sliced_wasserstein_loss on the float32 clouds xyz1 [B, N, 3] and
    xyz2 [B, M, 3] (each rows, or a view of channel planes: layout 1) and the
    contiguous float32 directions dirs [L, 3] (taken as given): loss_out [B] =
    the mean over the directions of the exact 1-D transport cost of the
    projections; slices (optional, contiguous [B, L]) = every direction's
    cost; gradxyz1 / gradxyz2 (each optional; its cloud's shape and layout) =
    the gradient of loss_out[bi] in that cloud; order1 / order2 (optional,
    contiguous int32 [B, L, N] / [B, L, M]) = the point of every rank."""
    optional = (slices, gradxyz1, gradxyz2, order1, order2)
    dev = _require_device(xyz1, xyz2, dirs, loss_out, *(t for t in optional if t is not None))
    _knn_cloud(xyz1, lay1, "sliced_wasserstein_loss")
    _knn_cloud(xyz2, lay2, "sliced_wasserstein_loss")
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if xyz2.shape[0] != b:
        raise ValueError("sliced_wasserstein_loss takes clouds of one batch size")
    if dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[1] != 3 or not dirs.is_contiguous():
        raise ValueError("dirs must be contiguous float32 of shape [L, 3]")
    l = dirs.shape[0]
    if loss_out.dtype != torch.float32 or tuple(loss_out.shape) != (b,) or not loss_out.is_contiguous():
        raise ValueError(f"loss_out must be contiguous float32 of shape {(b,)}")
    if slices is not None and (slices.dtype != torch.float32 or tuple(slices.shape) != (b, l)
                               or not slices.is_contiguous()):
        raise ValueError(f"slices must be contiguous float32 of shape {(b, l)}")
    for g, x, lay in ((gradxyz1, xyz1, lay1), (gradxyz2, xyz2, lay2)):
        if g is not None and (g.dtype != torch.float32 or g.shape != x.shape or cloud_layout(g) != int(lay)):
            raise ValueError("a gradient must have its cloud's dtype, shape and layout")
    for o, cnt in ((order1, n), (order2, m)):
        if o is not None and (o.dtype != torch.int32 or tuple(o.shape) != (b, l, cnt) or not o.is_contiguous()):
            raise ValueError(f"an order output must be contiguous int32 of shape {(b, l, cnt)}")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = sliced_workspace(dev, b, n, m, l)
        _check(load_library().pcm_sliced_wasserstein_loss(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), _ptr(dirs), l, _ptr(loss_out), _ptr(slices),
            _ptr(gradxyz1), _ptr(gradxyz2), _ptr(order1), _ptr(order2), _ptr(workspace), workspace.numel(),
            _stream(dev)), "pcm_sliced_wasserstein_loss")


CROSS_MAX_POINTS = 16384  # include/pcm.h PCM_CROSS_MAX_POINTS
CROSS_QUERIES = 1024  # query points per workgroup of csrc/chamfer_cross.hip (kCrossQW: 4 waves x 64 lanes x 4)
CROSS_TILE = 1024  # target points per LDS tile (kCrossTile)
CROSS_J = 8  # target clouds a workgroup streams past its queries, at most (kCrossJ)
CROSS_MIN_BLOCKS = 256  # the run is halved while the grid stays below this many workgroups (kCrossWantBlocks)


def chamfer_cross_run(s: int, r: int, n: int, m: int, both_dirs: bool = True) -> int:
    """Internal (tests): the target clouds per workgroup pcm_chamfer_cross takes
    at this shape: CROSS_J, halved while the grid stays below CROSS_MIN_BLOCKS."""
    return int(load_library().pcm_tune_chamfer_cross_run(int(s), int(r), int(n), int(m), int(bool(both_dirs))))


def chamfer_cross_workspace_bytes(s: int, r: int, n: int, m: int) -> int:
    return int(load_library().pcm_chamfer_cross_workspace_bytes(int(s), int(r), int(n), int(m)))


def chamfer_cross_workspace(dev: torch.device, s: int, r: int, n: int, m: int) -> torch.Tensor:
    """Scratch for chamfer_cross (a float64 record per entry, direction and
    workgroup of a query cloud): ONE buffer per (device, current stream), grown
    when a larger problem needs more; its content on entry is irrelevant and it
    holds nothing between calls."""
    need = max(chamfer_cross_workspace_bytes(s, r, n, m), 8)
    key = ("cross", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def chamfer_cross(xyz1, lay1, xyz2, lay2, mean12, mean21=None, workspace=None) -> None:
    """pcm_chamfer_cross on the float32 cloud sets xyz1 [S, N, 3] and xyz2
    [R, M, 3] (each rows, or a view of channel planes: layout 1): mean12 and,
    when given, mean21 (contiguous float32 [S, R]) = the mean nearest-neighbour
    squared distance of x_i's points to y_j and of y_j's points to x_i, both at
    [i, j] (include/pcm.h).  At most two launches."""
    outs = (mean12,) + (() if mean21 is None else (mean21,))
    dev = _require_device(xyz1, xyz2, *outs)
    _knn_cloud(xyz1, lay1, "chamfer_cross")
    _knn_cloud(xyz2, lay2, "chamfer_cross")
    s, n, r, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[0], xyz2.shape[1]
    for t in outs:
        if t.dtype != torch.float32 or tuple(t.shape) != (s, r) or not t.is_contiguous():
            raise ValueError(f"an output must be contiguous float32 of shape {(s, r)}")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = chamfer_cross_workspace(dev, s, r, n, m)
        _check(load_library().pcm_chamfer_cross(
            _ptr(xyz1), _ptr(xyz2), s, r, n, m, int(lay1), int(lay2), _ptr(mean12), _ptr(mean21), _ptr(workspace),
            workspace.numel(), _stream(dev)), "pcm_chamfer_cross")


CHAMFER_ND_MAX_DIM = 8  # include/pcm.h PCM_CHAMFER_ND_MAX_DIM
CHAMFER_ND_MAX_POINTS = 16384  # include/pcm.h PCM_CHAMFER_ND_MAX_POINTS
CHAMFER_ND_TILE = 1024  # candidates per LDS tile of csrc/chamfer_nd.hip (kNdTile)
CHAMFER_ND_QUERIES = 256  # queries per workgroup (kNdQB: 64 lanes x 4 a lane, held by every wave)
CHAMFER_ND_WAVES = 8  # waves that share a tile, an eighth each (kNdW)


def chamfer_nd_geometry():
    """Internal (tests): (tile, queries per workgroup, waves a tile) as the loaded library was compiled."""
    v = [ctypes.c_int(0) for _ in range(3)]
    load_library().pcm_tune_chamfer_nd_geometry(*[ctypes.addressof(x) for x in v])
    return tuple(x.value for x in v)


def cloud_layout_nd(t: torch.Tensor):
    """cloud_layout for a [B, N, D] cloud of any D >= 1: 0 for contiguous rows, 1 for
    a [B, N, D] view of a contiguous [B, D, N] tensor (channel planes), None for
    anything else.  A cloud that is both (D = 1 or N = 1) counts as rows."""
    if t.dim() != 3 or t.shape[2] < 1:
        return None
    if t.is_contiguous():
        return 0
    return 1 if t.transpose(1, 2).is_contiguous() else None


def _nd_clouds(x1, lay1, x2, lay2, what):
    if x1.dim() != 3 or x2.dim() != 3 or x1.shape[0] != x2.shape[0] or x1.shape[2] != x2.shape[2]:
        raise ValueError(f"{what} takes clouds [B, N, D] and [B, M, D] of one B and one D")
    if x1.dtype != torch.float32 or x2.dtype != torch.float32:
        raise TypeError(f"{what} takes float32 clouds")
    for t, lay in ((x1, lay1), (x2, lay2)):
        # a cloud that is rows and planes at once (one point, one coordinate) passes as either
        if lay not in (0, 1) or not (t.transpose(1, 2) if lay else t).is_contiguous():
            raise ValueError(f"{what}: a cloud is not in layout {lay} (rows 0, a view of channel planes 1)")
    b, n, d = x1.shape
    return b, n, x2.shape[1], d


def _nd_out(t, dtype, shape, what):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous {dtype} of shape {tuple(shape)}")


def chamfer_nd_forward(x1, lay1, x2, lay2, dist1, dist2, idx1, idx2) -> None:
    """pcm_chamfer_nd_forward on float32 clouds x1 [B, N, D] and x2 [B, M, D],
    1 <= D <= CHAMFER_ND_MAX_DIM, each rows (0) or a view of channel planes (1,
    cloud_layout_nd): dist float32 and idx int32, contiguous [B, N] / [B, M]."""
    dev = _require_device(x1, x2, dist1, dist2, idx1, idx2)
    b, n, m, d = _nd_clouds(x1, lay1, x2, lay2, "chamfer_nd_forward")
    for t, dt, k in ((dist1, torch.float32, n), (dist2, torch.float32, m), (idx1, torch.int32, n),
                     (idx2, torch.int32, m)):
        _nd_out(t, dt, (b, k), "a chamfer_nd_forward output")
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_nd_forward(
            _ptr(x1), _ptr(x2), b, n, m, d, int(lay1), int(lay2), _ptr(dist1), _ptr(dist2), _ptr(idx1), _ptr(idx2),
            _stream(dev)), "pcm_chamfer_nd_forward")


def chamfer_nd_backward(x1, lay1, x2, lay2, graddist1, graddist2, idx1, idx2, grad1, grad2) -> None:
    """pcm_chamfer_nd_backward: grad1 / grad2 (float32, shaped and laid out as
    their clouds) fully overwritten; graddists float32 and indices int32,
    contiguous [B, N] / [B, M]."""
    dev = _require_device(x1, x2, graddist1, graddist2, idx1, idx2, grad1, grad2)
    b, n, m, d = _nd_clouds(x1, lay1, x2, lay2, "chamfer_nd_backward")
    _nd_clouds(grad1, lay1, grad2, lay2, "chamfer_nd_backward (gradients)")
    if tuple(grad1.shape) != tuple(x1.shape) or tuple(grad2.shape) != tuple(x2.shape):
        raise ValueError("chamfer_nd_backward: a gradient is not shaped as its cloud")
    for t, dt, k in ((graddist1, torch.float32, n), (graddist2, torch.float32, m), (idx1, torch.int32, n),
                     (idx2, torch.int32, m)):
        _nd_out(t, dt, (b, k), "a chamfer_nd_backward graddist / index")
    with torch.cuda.device(dev):
        _check(load_library().pcm_chamfer_nd_backward(
            _ptr(x1), _ptr(x2), b, n, m, d, int(lay1), int(lay2), _ptr(graddist1), _ptr(graddist2), _ptr(idx1),
            _ptr(idx2), _ptr(grad1), _ptr(grad2), _stream(dev)), "pcm_chamfer_nd_backward")


DCD_MAX_POINTS = 16384  # include/pcm.h PCM_DCD_MAX_POINTS


def dcd_workspace_bytes(b: int, n: int, m: int) -> int:
    return int(load_library().pcm_dcd_workspace_bytes(int(b), int(n), int(m)))


def dcd_workspace(dev: torch.device, b: int, n: int, m: int) -> torch.Tensor:
    """Scratch for dcd_loss (the forward's distances and argmins, the grid
    forward's own bytes for large clouds, the graddists and a gradient each):
    ONE buffer per (device, current stream), grown when a larger problem needs
    more; its content on entry is irrelevant and it holds nothing between
    calls."""
    need = max(dcd_workspace_bytes(b, n, m), 16)
    key = ("dcd", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def dcd_loss(xyz1, lay1, xyz2, lay2, alpha, n_lambda, non_reg, loss_out, cd=None, gradxyz1=None, gradxyz2=None,
             count1=None, count2=None, graddist1=None, graddist2=None, workspace=None) -> None:
    """pcm_dcd_loss on the float32 clouds xyz1 [B, N, 3] and xyz2 [B, M, 3]
    (each rows, or a view of channel planes: layout 1): loss_out [B] = the
    density-aware Chamfer distance at ``alpha`` and ``n_lambda``; cd
    (optional, contiguous [B, 2]) = cd_p and cd_t; gradxyz1 / gradxyz2 (each
    optional; its cloud's shape and layout) = the gradient of loss_out[bi] in
    that cloud; count1 / count2 (optional, contiguous int32 [B, N] / [B, M]) =
    how many points of the other cloud have each point as their neighbour;
    graddist1 / graddist2 (optional, contiguous [B, N] / [B, M]) = the
    per-point weights the Chamfer backward is fed."""
    optional = (cd, gradxyz1, gradxyz2, count1, count2, graddist1, graddist2)
    dev = _require_device(xyz1, xyz2, loss_out, *(t for t in optional if t is not None))
    _knn_cloud(xyz1, lay1, "dcd_loss")
    _knn_cloud(xyz2, lay2, "dcd_loss")
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if xyz2.shape[0] != b:
        raise ValueError("dcd_loss takes clouds of one batch size")
    if loss_out.dtype != torch.float32 or tuple(loss_out.shape) != (b,) or not loss_out.is_contiguous():
        raise ValueError(f"loss_out must be contiguous float32 of shape {(b,)}")
    if cd is not None and (cd.dtype != torch.float32 or tuple(cd.shape) != (b, 2) or not cd.is_contiguous()):
        raise ValueError(f"cd must be contiguous float32 of shape {(b, 2)}")
    for g, x, lay in ((gradxyz1, xyz1, lay1), (gradxyz2, xyz2, lay2)):
        if g is not None and (g.dtype != torch.float32 or g.shape != x.shape or cloud_layout(g) != int(lay)):
            raise ValueError("a gradient must have its cloud's dtype, shape and layout")
    for t, dtype, cnt in ((count1, torch.int32, n), (count2, torch.int32, m), (graddist1, torch.float32, n),
                          (graddist2, torch.float32, m)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (b, cnt) or not t.is_contiguous()):
            raise ValueError(f"a per-point output must be contiguous {dtype} of shape {(b, cnt)}")
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = dcd_workspace(dev, b, n, m)
        _check(load_library().pcm_dcd_loss(
            _ptr(xyz1), _ptr(xyz2), b, n, m, int(lay1), int(lay2), float(alpha), float(n_lambda), int(bool(non_reg)),
            _ptr(loss_out), _ptr(cd), _ptr(gradxyz1), _ptr(gradxyz2), _ptr(count1), _ptr(count2), _ptr(graddist1),
            _ptr(graddist2), _ptr(workspace), workspace.numel(), _stream(dev)), "pcm_dcd_loss")


def emd_workspace_bytes(b: int, n: int) -> int:
    return int(load_library().pcm_emd_workspace_bytes(b, n))


def emd_workspace(dev: torch.device, b: int, n: int) -> torch.Tensor:
    """EMD workspace cached per (device, current stream, size); its content on
    entry is irrelevant, but a call's auction state lives in it until the call
    ends, so concurrent calls on different streams get different buffers."""
    ws_bytes = max(emd_workspace_bytes(b, n), 1)
    key = ("emd", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < ws_bytes:  # one per (device, stream), grown when needed
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def emd_forward(xyz1, xyz2, eps: float, iters: int, dist, assignment, price=None,
                workspace=None, helpers=None, offload_min=None, stats=None, diag=1, wsplit=None,
                tail_max=None, spin_limit=None) -> None:
    """pcm_emd_forward; helpers / offload_min / stats select the tuning entry
    (helper workgroups per cloud, the miss count above which an iteration's
    full scans are offloaded, diagnostics of kind `diag`: 1 counts, 2 + i phase
    timers of batch element i; wsplit: waves per few-miss full scan; tail_max:
    bidders at or below which an iteration runs in tail mode, 0 = never;
    spin_limit: bound of the waits between workgroups, 0 forces the timeout
    path -- csrc/emd.hip pcm_tune_emd_forward_cfg) -- None = the defaults."""
    dev = _require_device(xyz1, xyz2, dist, assignment)
    b, n, _ = xyz1.shape
    ws_bytes = emd_workspace_bytes(b, n)
    if ws_bytes and (workspace is None or workspace.numel() * workspace.element_size() < ws_bytes):
        workspace = emd_workspace(dev, b, n)
    with torch.cuda.device(dev):
        if (helpers is None and offload_min is None and stats is None and wsplit is None and tail_max is None
                and spin_limit is None):
            _check(load_library().pcm_emd_forward(
                _ptr(xyz1), _ptr(xyz2), b, n, float(eps), int(iters), _ptr(dist), _ptr(assignment),
                _ptr(price), _ptr(workspace), ws_bytes, _stream(dev)), "pcm_emd_forward")
        else:
            if stats is not None and stats.numel() < 3 * int(iters) + 16 + b:
                raise ValueError("stats needs 3*iters + 16 + B int32 entries")
            _check(load_library().pcm_tune_emd_forward_cfg(
                _ptr(xyz1), _ptr(xyz2), b, n, float(eps), int(iters), _ptr(dist), _ptr(assignment),
                _ptr(price), _ptr(workspace), ws_bytes, -1 if helpers is None else int(helpers),
                -1 if offload_min is None else int(offload_min), int(diag), 0 if wsplit is None else int(wsplit),
                -1 if tail_max is None else int(tail_max), -1 if spin_limit is None else int(spin_limit),
                _ptr(stats), _stream(dev)),
                "pcm_tune_emd_forward_cfg")


def emd_workspace_status(workspace, b: int, n: int) -> None:
    """Raise PcmError if reading the last EMD forward's status fails
    (synchronises the current stream).  A helper job that timed out is not an
    error: the master scanned those items itself (emd_timeouts counts them)."""
    dev = workspace.device
    with torch.cuda.device(dev):
        _check(load_library().pcm_emd_workspace_status(_ptr(workspace), workspace.numel(), b, n, _stream(dev)),
               "pcm_emd_workspace_status")


def emd_timeouts(workspace, b: int, n: int) -> int:
    """Internal: batch elements of the last EMD forward on `workspace` whose
    master timed out on a helper job and scanned the items itself."""
    dev = workspace.device
    with torch.cuda.device(dev):
        r = int(load_library().pcm_tune_emd_timeouts(_ptr(workspace), workspace.numel(), b, n, _stream(dev)))
    if r < 0:
        _check(r, "pcm_tune_emd_timeouts")
    return r


def emd_backward(xyz1, xyz2, graddist, assignment, gradxyz1) -> None:
    dev = _require_device(xyz1, xyz2, graddist, assignment, gradxyz1)
    b, n, _ = xyz1.shape
    with torch.cuda.device(dev):
        _check(load_library().pcm_emd_backward(
            _ptr(xyz1), _ptr(xyz2), b, n, _ptr(graddist), _ptr(assignment), _ptr(gradxyz1),
            _stream(dev)), "pcm_emd_backward")


def _nn_workspace(dev, b: int, m: int):
    """Cached workspace for the screening rows (content on entry irrelevant)."""
    need = max(int(load_library().pcm_icp_workspace_bytes(b, m)), 1)
    key = ("nn", dev, _stream_id(dev))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _cache_put(key, ws)
    return _hand_out(ws)


def icp(A, B, init_pose, max_iterations: int, tolerance: float, T_out, distances, iterations,
        workspace=None) -> None:
    """pcm_icp on float64 device tensors A, B [b,n,3], init_pose None or [b,4,4];
    outputs T_out [b,4,4] float64, distances [b,n] float64, iterations [b] int32."""
    dev = _require_device(A, B, T_out, distances, iterations)
    b, n, _ = A.shape
    if workspace is None:
        workspace = _nn_workspace(dev, b, n)
    with torch.cuda.device(dev):
        _check(load_library().pcm_icp(
            _ptr(A), _ptr(B), b, n, _ptr(init_pose), int(max_iterations), float(tolerance), _ptr(T_out),
            _ptr(distances), _ptr(iterations), _ptr(workspace), workspace.numel(), _stream(dev)), "pcm_icp")


def icp_workspace_status(workspace, b: int, n: int) -> None:
    """Raise PcmError if the last pcm_icp on `workspace` hit a device-side
    timeout between the workgroups of a pair (synchronises the current stream)."""
    dev = workspace.device
    with torch.cuda.device(dev):
        _check(load_library().pcm_icp_workspace_status(_ptr(workspace), workspace.numel(), b, n, _stream(dev)),
               "pcm_icp_workspace_status")


def nearest_neighbor(src, dst, distances, indices, workspace=None) -> None:
    """pcm_nearest_neighbor on float64 device tensors src [b,n,3], dst [b,m,3]."""
    dev = _require_device(src, dst, distances, indices)
    b, n, _ = src.shape
    m = dst.shape[1]
    if workspace is None:
        workspace = _nn_workspace(dev, b, m)
    with torch.cuda.device(dev):
        _check(load_library().pcm_nearest_neighbor(
            _ptr(src), _ptr(dst), b, n, m, _ptr(distances), _ptr(indices), _ptr(workspace), workspace.numel(),
            _stream(dev)), "pcm_nearest_neighbor")


def best_fit_transform(A, B, T_out) -> None:
    """pcm_best_fit_transform on float64 device tensors A, B [b,n,3] -> T_out [b,4,4]."""
    dev = _require_device(A, B, T_out)
    b, n, _ = A.shape
    with torch.cuda.device(dev):
        _check(load_library().pcm_best_fit_transform(_ptr(A), _ptr(B), b, n, _ptr(T_out), _stream(dev)),
               "pcm_best_fit_transform")
