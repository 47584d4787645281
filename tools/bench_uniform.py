#!/usr/bin/env python3
"""The uniform-loss step: the library's one call against the composed sequence
it replaces, alternated in one process on the same GPU.

  (A) composed: farthest point seeds (sampling: pcm_fps) and their gather; per
      percentage a ball query in torch (torch.cdist, a comparison, cumulative
      counts and a scatter into the first nsample slots, the first hit behind
      them), pointnet2_utils.grouping_operation, knn.KNN(2) of every group
      against itself; then a differentiable torch recomputation of the chosen
      distances, the loss and backward;
  (B) loss.Loss().get_uniform_loss(x).backward(): pcm_uniform_loss
      (csrc/grouping.hip) and the scaling of its gradient;
  (B') pcm_hip.uniform_loss alone, loss and gradient: what (B) enqueues but for
      that scaling, and the form that is captured.

At B=32 and B=128, N=1024, the default percentages.  Per sequence (the helpers
are tools/bench_fps.py's):
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise, median of `rounds` rounds in which the sequences alternate
            (every sequence warmed at the timed shape first);
  graph us  ten back-to-back calls captured once and replayed, per call ((B') only);
  kernels   device kernels per call, counted by torch.profiler in an untimed pass.
The sequences' results are compared before timing.  One JSON line at the end.

    python tools/bench_uniform.py [--rounds 5] [--quick]
"""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "utils"), os.path.join(PKG, "loss"),
          os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcm_hip  # noqa: E402
import knn  # noqa: E402
import loss as loss_mod  # noqa: E402
import pointnet2_utils as pn2  # noqa: E402
import sampling  # noqa: E402
from bench_fps import measure  # noqa: E402

SHAPES = [(32, 1024), (128, 1024)]  # (B, N)
PERCENTAGE = [0.004, 0.006, 0.008, 0.010, 0.012]
RADIUS = 1.0


def torch_ball_query(radius, nsample, xyz, new_xyz):
    """The ball query as torch ops: the first nsample points, in index order,
    closer to a centre than radius; the first hit behind them; zeros without one."""
    b, n, _ = xyz.shape
    s = new_xyz.shape[1]
    inside = torch.cdist(new_xyz, xyz) < radius
    rank = inside.cumsum(-1)
    keep = inside & (rank <= nsample)
    first = inside.int().argmax(-1)  # 0 without a hit
    out = first.unsqueeze(-1).repeat(1, 1, nsample + 1)
    point = torch.arange(n, device=xyz.device).view(1, 1, n).expand(b, s, n)
    out.scatter_(2, torch.where(keep, rank - 1, nsample), point)  # a point that is not kept lands in the spare column
    return out[:, :, :nsample].contiguous()


def composed(xyz, search):
    """Sequence (A): loss and gradient through the separate operations."""
    x = xyz.detach().requires_grad_(True)
    b, n, _ = x.shape
    npoint = int(n * 0.05)
    seeds, new_xyz = sampling.sample_points(x.detach(), npoint)
    feats = x.transpose(1, 2).contiguous()
    expect_len = math.sqrt(math.pi * RADIUS ** 2 / n)
    total = 0
    for p in PERCENTAGE:
        nsample = int(n * p)
        idx = torch_ball_query(math.sqrt(p * RADIUS), nsample, x.detach(), new_xyz)
        grouped = pn2.grouping_operation(feats, idx).permute(0, 2, 3, 1).reshape(b * npoint, nsample, 3)
        _, near = search(grouped.detach().contiguous(), grouped.detach().contiguous())
        other = torch.gather(grouped, 1, near[:, :, 1:2].clamp(min=0).expand(-1, -1, 3))
        sq = (grouped - other).pow(2).sum(-1)
        live = sq > 0  # a zero distance (a padding copy) has no finite derivative: it adds 1e-8 and no gradient
        dist = torch.where(live, torch.sqrt(torch.where(live, sq, torch.ones_like(sq))), torch.zeros_like(sq))
        m = (dist + 1e-8).mean(1)
        total = total + ((m - expect_len) ** 2 / (expect_len + 1e-8)).mean() * (p * 100) ** 2
    value = total / len(PERCENTAGE)
    value.backward()
    return value.detach(), x.grad


def show(title, res, note=""):
    fmt = lambda v: "      n/a" if v is None else f"{v:9.2f}"  # noqa: E731
    print(title, flush=True)
    for key, (label, r) in res.items():
        print(f"  {label:40s}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]  graph "
              f"{fmt(r['graph_us'])} us  kernels/call {r['kernels']}", flush=True)
    if note:
        print("  " + note, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_uniform needs a HIP device")
    dev = torch.device("cuda:0")
    search = knn.KNN(k=2, transpose_mode=True)
    module = loss_mod.Loss()
    results = []
    for b, n in SHAPES:
        g = torch.Generator().manual_seed(7)
        # a thin shell: its groups are padded, full and truncated (a cube's are nearly all padded at this size)
        dirs = torch.randn(b, n, 3, generator=g)
        xyz = (0.5 * dirs / dirs.norm(dim=2, keepdim=True)).to(dev)
        npoint = int(n * 0.05)
        nsample = [int(n * p) for p in PERCENTAGE]
        radii = [math.sqrt(p * RADIUS) for p in PERCENTAGE]
        weight = [(p * 100) ** 2 / len(PERCENTAGE) for p in PERCENTAGE]
        expect_len = math.sqrt(math.pi * RADIUS ** 2 / n)
        loss = torch.empty(1, device=dev)
        grad = torch.empty_like(xyz)

        def fused():
            x = xyz.detach().requires_grad_(True)
            module.get_uniform_loss(x, PERCENTAGE, RADIUS).backward()
            return x.grad

        def kernel_only():
            pcm_hip.uniform_loss(xyz, 0, npoint, nsample, radii, weight, expect_len, loss, grad)

        fns = {"a": lambda: composed(xyz, search), "b": fused, "bk": kernel_only}
        # the sequences agree before anything is timed; torch's differently rounded cdist may move a
        # point across a sphere, so the difference is shown, not hidden
        la, ga = composed(xyz, search)
        gb = fused()
        kernel_only()
        torch.cuda.synchronize()
        assert torch.equal(gb, grad)
        loss_rel = abs(loss.item() - la.item()) / abs(la.item())
        grad_rel = float((grad - ga).abs().max() / ga.abs().max())
        reps = {"a": 10 if not args.quick else 1, "b": 100 if not args.quick else 2,
                "bk": 100 if not args.quick else 2}
        res = measure(fns, reps, args.rounds, capturable=["bk"])
        row = dict(what="uniform", b=b, n=n, percentage=PERCENTAGE, rounds=args.rounds, loss_rel_diff=loss_rel,
                   grad_rel_diff=grad_rel, sequences=res, speedup_eager=res["a"]["us"] / res["b"]["us"])
        results.append(row)
        show(f"uniform step B={b} N={n}  (loss differs from the composed one by {loss_rel:.1e}, gradient by "
             f"{grad_rel:.1e} of its largest entry)",
             {"a": ("(A) composed sequence and backward", res["a"]),
              "b": ("(B) get_uniform_loss and backward", res["b"]),
              "bk": ("(B') pcm_uniform_loss, loss and gradient", res["bk"])},
             f"(A) / (B) eager: {row['speedup_eager']:.2f}x")
    print(json.dumps({"tool": "bench_uniform", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
