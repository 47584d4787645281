"""The pinned arithmetic of the one-pass Chamfer evaluation (include/pcm.h,
pcm_chamfer_eval) in numpy, shared by tests/test_fscore_gpu.py and the F-score
op of tests/test_geometry_cpu.py / tests/test_geometry_gpu.py: strict counts
under float32 thresholds, the float32 scores on those counts and the
sequential batch mean."""
import numpy as np


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def counts_from(d, ths):
    """[B, T] counts of d [B, P] (float32) strictly under each float32 threshold."""
    th = np.asarray(ths, np.float32)
    return (d[:, None, :] < th[None, :, None]).sum(-1).astype(np.int32)


def scores_from(c1, c2, n, m):
    """The pinned arithmetic of include/pcm.h in float32."""
    p_x = c1.astype(np.float32) / np.float32(n)
    p_y = c2.astype(np.float32) / np.float32(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = ((np.float32(2) * p_y) * p_x) / (p_y + p_x)
    f = np.where(c1 + c2 == 0, np.float32(0), f).astype(np.float32)
    return np.stack([f, p_x, p_y], -1)


def batch_from(scores):
    s = np.zeros(scores.shape[1:], np.float32)
    for i in range(scores.shape[0]):  # sequential, ascending b
        s = s + scores[i]
    return s / np.float32(scores.shape[0])
