#!/usr/bin/env python3
"""k nearest neighbours and the repulsion step: the library's kernels against
torch's own sequence, alternated in one process.

  knn        (A) torch.cdist, square, topk(largest=False);
             (B) knn.knn_points: pcm_knn (csrc/knn.hip), one launch -- and its kernel
                 forms forced through pcm_tune_knn: one wave per 64 queries that ballots
                 and inserts at once (b1), one wave with per-lane queues (b2), the queued
                 form with the reference cloud split over four waves (b3);
             at k = 5 and k = 20, B=32 N=M=1024 and B=8 N=M=16384 (self search).
  repulsion  (A) torch.cdist, square, topk(largest=False), gather, clamp, mean and
                 backward;
             (B) pcm_repulsion_loss: loss and gradient from one call;
             at B=32 N=1024, h = 0.004.

Per shape and sequence (the helpers are tools/bench_fps.py's):
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise, median of `rounds` rounds in which the sequences alternate
            (every sequence warmed at the timed shape first);
  graph us  ten back-to-back calls captured once and replayed, per call; the torch
            sequences are timed eagerly only;
  kernels   device kernels per call, counted by torch.profiler in an untimed pass.
The sequences' results are compared before timing.  One JSON line at the end.

    python tools/bench_knn.py [--rounds 5] [--quick]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "utils"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcm_hip  # noqa: E402
import knn  # noqa: E402
from bench_fps import measure  # noqa: E402

KNN_SHAPES = [(32, 1024), (8, 16384)]  # (B, N): a self search
KNN_KS = [5, 20]
REPULSION_SHAPE = (32, 1024, 0.004)  # (B, N, h): about a quarter of the terms active on a uniform cloud


def torch_knn(xyz, k):
    """Sequence (A): the distance matrix, its square, the k smallest per row."""
    return torch.cdist(xyz, xyz).pow(2).topk(k, dim=-1, largest=False)


def torch_repulsion(xyz, h):
    """Sequence (A): cdist, square, topk, gather, clamp, mean and backward."""
    x = xyz.detach().requires_grad_(True)
    d = torch.cdist(x, x).pow(2)
    idx = d.detach().topk(5, dim=-1, largest=False)[1]
    loss = torch.clamp(h - d.gather(2, idx)[:, :, 1:], min=0).mean()
    loss.backward()
    return loss.detach(), x.grad


def show(title, res, note=""):
    fmt = lambda v: "      n/a" if v is None else f"{v:9.2f}"  # noqa: E731
    print(title, flush=True)
    for key, (label, r) in res.items():
        print(f"  {label:34s}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]  graph "
              f"{fmt(r['graph_us'])} us  kernels/call {r['kernels']}", flush=True)
    if note:
        print("  " + note, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn needs a HIP device")
    dev = torch.device("cuda:0")
    results = []

    for b, n in KNN_SHAPES:
        g = torch.Generator().manual_seed(7)
        xyz = torch.rand(b, n, 3, generator=g).to(dev)
        for k in KNN_KS:
            dist = torch.empty(b, n, k, device=dev)
            idx = torch.empty(b, n, k, dtype=torch.int32, device=dev)

            def forced(variant):
                return lambda: pcm_hip.knn(xyz, 0, xyz, 0, k, dist, idx, variant=variant)

            fns = {"a": lambda: torch_knn(xyz, k), "b": lambda: knn.knn_points(xyz, xyz, k), "b1": forced(1),
                   "b2": forced(2), "b3": forced(3)}
            # the sequences agree before anything is timed: the forced variants bit for bit, torch's rows
            # where its differently rounded distances order the same (counted, not hidden)
            want_d, want_i = knn.knn_points(xyz, xyz, k)
            for key in ("b1", "b2", "b3"):
                fns[key]()
                assert torch.equal(idx, want_i) and torch.equal(dist.view(torch.int32), want_d.view(torch.int32)), key
            ta = torch_knn(xyz, k)
            same_rows = int((ta[1] == want_i.long()).all(-1).sum())
            del ta
            torch.cuda.synchronize()
            big = n > 4096
            ours = (20 if big else 200) if not args.quick else 2
            theirs = (2 if big else 20) if not args.quick else 1
            reps = {key: (theirs if key == "a" else ours) for key in fns}
            res = measure(fns, reps, args.rounds, capturable=["b1", "b2", "b3"])
            labels = {"a": "(A) cdist, square, topk", "b": "(B) knn_points", "b1": "    one wave, insert at once",
                      "b2": "    one wave, queued", "b3": "    four waves, queued"}
            picked = "b3" if pcm_hip.knn_default_split(b, n) > 1 else "b2"
            labels[picked] += " (picked)"
            best = res[picked]["graph_us"] or res[picked]["us"]
            row = dict(what="knn", b=b, n=n, k=k, rounds=args.rounds, rows_equal_to_torch=same_rows,
                       rows=b * n, sequences=res, speedup_eager=res["a"]["us"] / res["b"]["us"],
                       pairs_per_us=b * n * n / best)
            results.append(row)
            show(f"knn B={b} N=M={n} k={k}  ({same_rows}/{b * n} rows equal to torch's)",
                 {key: (labels[key], r) for key, r in res.items()},
                 f"(A) / (B) eager: {row['speedup_eager']:.2f}x; {row['pairs_per_us']:.0f} pairs per us (the picked form, graph)")

    b, n, h = REPULSION_SHAPE
    g = torch.Generator().manual_seed(7)
    xyz = torch.rand(b, n, 3, generator=g).to(dev)
    loss = torch.empty(1, device=dev)
    grad = torch.empty_like(xyz)
    fns = {"a": lambda: torch_repulsion(xyz, h), "b": lambda: pcm_hip.repulsion_loss(xyz, 0, h, loss, grad)}
    la, ga = torch_repulsion(xyz, h)
    fns["b"]()
    torch.cuda.synchronize()
    loss_rel = abs(loss.item() - la.item()) / abs(la.item())
    grad_err = float((grad - ga).abs().max() / ga.abs().max())
    reps = {"a": 20 if not args.quick else 1, "b": 200 if not args.quick else 2}
    res = measure(fns, reps, args.rounds, capturable=["b"])
    row = dict(what="repulsion", b=b, n=n, h=h, rounds=args.rounds, loss_rel_diff=loss_rel, grad_rel_diff=grad_err,
               sequences=res, speedup_eager=res["a"]["us"] / res["b"]["us"])
    results.append(row)
    show(f"repulsion step B={b} N={n} h={h}  (loss differs from torch's by {loss_rel:.1e}, gradient by {grad_err:.1e})",
         {"a": ("(A) torch sequence and backward", res["a"]), "b": ("(B) pcm_repulsion_loss", res["b"])},
         f"(A) / (B) eager: {row['speedup_eager']:.2f}x")
    print(json.dumps({"tool": "bench_knn", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
