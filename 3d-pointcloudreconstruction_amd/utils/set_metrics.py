"""Set-level metrics on cross Chamfer matrices: nearest-shape retrieval,
MMD-CD, COV-CD and 1-NNA-CD.

The matrices come from cross_chamfer_3D.chamfer_cross (pcm_chamfer_cross, one
call a matrix); everything here is plain torch on those small [S, R] tensors
and runs wherever they live.  Every tie goes to the LOWEST index: the minima
are taken with torch.min(dim), which is documented to return the index of the
first minimal value.

Definitions (Achlioptas et al., "Learning Representations and Generative Models
for 3D Point Clouds", ICML 2018; Yang et al., "PointFlow", ICCV 2019), for a
set of S generated samples and R reference clouds and cd[i, j] the Chamfer
distance of sample i to reference j:
  MMD-CD   = mean over references j of min over samples i of cd[i, j];
  COV-CD   = #{distinct j : j = argmin_j' cd[i, j'] for some sample i} / R;
  1-NNA-CD = the leave-one-out accuracy of the 1-nearest-neighbour classifier
             on the union of both sets (samples labelled 0, references 1) under
             the (S+R) x (S+R) matrix [[cd_ss, cd_sr], [cd_sr^T, cd_rr]] with its
             diagonal excluded; 0.5 is the best a generator can score.
The formulas are stated from the publications, not verified against their
packages (neither is installed where this was written); this text is the
contract.  The means are taken in float64 of the float32 entries.
"""
import os
import sys

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_PKG, "metric"), os.path.join(_PKG, "metric", "chamfer3D")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _matrix(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point():
        raise ValueError(f"{name} must be a floating-point matrix")
    return t


def nearest_shape(query, gallery):
    """(idx [S] int64, cd [S]): for every cloud of query [S, N, 3] the cloud of
    gallery [R, M, 3] of least Chamfer distance (mean12 + mean21 of
    chamfer_cross) and that distance; ties go to the lowest gallery index."""
    from cross_chamfer_3D import chamfer_cross
    if gallery.size(0) == 0:
        raise ValueError("nearest_shape needs a gallery of at least one cloud")
    cd, idx = torch.min(chamfer_cross(query, gallery).cd, dim=1)
    return idx, cd


def mmd_cov(cd):
    """(MMD-CD, COV-CD) as Python floats for cd [S, R] (samples x references)."""
    cd = _matrix(cd, "cd")
    s, r = cd.shape
    if s == 0 or r == 0:
        raise ValueError("mmd_cov needs at least one sample and one reference")
    mmd = torch.min(cd, dim=0).values.double().mean()
    nearest = torch.min(cd, dim=1).indices  # each sample's nearest reference
    hit = torch.zeros(r, dtype=torch.bool, device=cd.device)
    hit[nearest] = True
    return float(mmd), float(hit.sum()) / r


def one_nna(cd_ss, cd_sr, cd_rr):
    """The leave-one-out 1-nearest-neighbour accuracy (a Python float) for the
    matrices cd_ss [S, S], cd_sr [S, R] and cd_rr [R, R]."""
    cd_ss, cd_sr, cd_rr = _matrix(cd_ss, "cd_ss"), _matrix(cd_sr, "cd_sr"), _matrix(cd_rr, "cd_rr")
    s, r = cd_sr.shape
    if tuple(cd_ss.shape) != (s, s) or tuple(cd_rr.shape) != (r, r):
        raise ValueError("one_nna takes cd_ss [S, S], cd_sr [S, R] and cd_rr [R, R]")
    if s + r < 2:
        raise ValueError("one_nna needs at least two clouds")
    full = torch.cat([torch.cat([cd_ss, cd_sr], dim=1), torch.cat([cd_sr.t(), cd_rr], dim=1)], dim=0).clone()
    full.fill_diagonal_(float("inf"))
    nearest = torch.min(full, dim=1).indices
    label = torch.cat([torch.zeros(s, dtype=torch.long), torch.ones(r, dtype=torch.long)]).to(full.device)
    return float((label[nearest] == label).double().mean())


def compute_set_metrics(sample, ref):
    """{'MMD-CD', 'COV-CD', '1-NNA-CD'} for the generated clouds sample
    [S, N, 3] and the reference clouds ref [R, M, 3]: three chamfer_cross
    calls, one across the sets and one of each set with itself."""
    from cross_chamfer_3D import chamfer_cross
    cd_sr = chamfer_cross(sample, ref).cd
    cd_ss = chamfer_cross(sample).cd
    cd_rr = chamfer_cross(ref).cd
    mmd, cov = mmd_cov(cd_sr)
    return {"MMD-CD": mmd, "COV-CD": cov, "1-NNA-CD": one_nna(cd_ss, cd_sr, cd_rr)}
