#!/usr/bin/env python3
"""Projection loss: the silhouette kernels against a torch restatement of the
reference's op sequence, alternated in one process.

  (A) the reference's ops on the device, restated here: cont_proj's broadcast
      difference [B, N, H, W, 2], exp, product, sum over N
      (utils/projection.py:52-64), then the elementwise 'bce_prob' loss and its
      mean (loss/proj_loss.py:17-19, :43) and autograd's backward to the cloud.
      (The reference itself runs cont_proj on the CPU, utils/utils.py:232.)
      B=32 only: each of its B x N x H x W x 2 tensors is 1 GiB there.
  (B) projection.cont_proj and proj_loss.get_loss_proj(.., 'bce_prob'):
      pcm_silhouette_forward / pcm_proj_bce / pcm_silhouette_backward
      (csrc/silhouette.hip).

Shapes: N=1024, 64x64, sigma_sq=2 (finetune.py:37-39) at B=32 and B=128
(finetune.py:40).  Timed per setting and sequence, `forward` (cont_proj of the
predicted clouds) and `step` (that silhouette, the loss against a fixed
ground-truth silhouette, and the backward to the cloud):
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise (what a training loop pays, launch gaps included),
            median of `rounds` rounds in which A and B alternate;
  graph us  ten back-to-back calls captured once and replayed, per call
            (device time without the host's enqueue cost; a replay's own
            fixed cost is shared by the ten);
  kernels   device kernels per call, counted by torch.profiler in an untimed pass;
and for (B)'s forward the time against its VALU floor: B N H W fused
multiply-adds at two per packed lane operation over 78.6 T lane-op/s.
Both sequences' silhouettes, losses and gradients are compared before timing.
One JSON line at the end.

    python tools/bench_silhouette.py [--rounds 5] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "utils"), os.path.join(PKG, "loss")):
    if p not in sys.path:
        sys.path.insert(0, p)
import proj_loss  # noqa: E402
import projection  # noqa: E402

LANE_OPS_PER_S = 78.6e12  # packed-fp32 VALU lane operations per second
N, H, W, SIGMA_SQ = 1024, 64, 64, 2.0


def torch_cont_proj(pcl, grid_h, grid_w, sigma_sq):
    """projection.py:18-64 on pcl's device."""
    x = (pcl[:, :, 0:1] + 1) * grid_h / 2
    y = (pcl[:, :, 1:2] + 1) * grid_w / 2
    pcl_xy = torch.cat([x, y], 2)
    gh, gw = torch.meshgrid(torch.arange(grid_h, dtype=torch.float32, device=pcl.device),
                            torch.arange(grid_w, dtype=torch.float32, device=pcl.device), indexing="ij")
    grid_xy = torch.stack([gh, gw], 2)
    diff = pcl_xy[:, :, None, None, :] - grid_xy  # [B, N, H, W, 2]
    val = torch.exp(-(diff ** 2) / (2. * sigma_sq))
    val = val[:, :, :, :, 0] * val[:, :, :, :, 1]
    return torch.sum(val, 1)


def torch_bce_prob(pred, gt, w=1.0):
    """proj_loss.py:17-19 and the mean of :43."""
    epsilon = 1e-8
    loss = -gt * torch.log(pred + epsilon) * w - (1 - gt) * torch.log(torch.abs(1 - pred - epsilon))
    return torch.mean(loss)


def eager_us(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / reps


GRAPH_CALLS = 10  # calls per captured graph: a replay's fixed host cost is shared by ten calls


def captured(fn):
    """A graph of GRAPH_CALLS back-to-back calls, or None where the sequence cannot be captured."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_CALLS):
                fn()
        g.replay()
        torch.cuda.synchronize()
        return g
    except Exception as e:  # noqa: BLE001
        print(f"    (not capturable: {type(e).__name__}: {e})", flush=True)
        torch.cuda.synchronize()
        return None


def kernels_per_call(fn, calls=3):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n / calls
    except Exception as e:  # noqa: BLE001
        print(f"    (kernel count unavailable: {type(e).__name__}: {e})", flush=True)
        return None


def measure(fns, reps, rounds):
    """{name: dict(us, us_min, us_max, graph_us, kernels)} with the sequences alternated per round."""
    for _ in range(2):  # warm-up of every sequence at the timed shape
        for fn in fns.values():
            eager_us(fn, max(2, reps // 4))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(eager_us(fn, reps))
    graphs = {k: captured(fn) for k, fn in fns.items()}
    gtimes = {k: [] for k in fns}
    for _ in range(rounds):
        for k, g in graphs.items():
            if g is not None:
                gtimes[k].append(eager_us(g.replay, max(2, reps // GRAPH_CALLS)) / GRAPH_CALLS)
    out = {}
    for k, fn in fns.items():
        out[k] = dict(us=statistics.median(times[k]), us_min=min(times[k]), us_max=max(times[k]),
                      graph_us=statistics.median(gtimes[k]) if gtimes[k] else None,
                      graph_us_min=min(gtimes[k]) if gtimes[k] else None,
                      graph_us_max=max(gtimes[k]) if gtimes[k] else None,
                      kernels=kernels_per_call(fn))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="only run this many eager (B) steps per batch size, untimed: the workload for a "
                         "kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_silhouette.py "
                         "--trace-steps 30)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_silhouette needs a HIP device")
    dev = torch.device("cuda:0")
    if args.trace_steps:
        for b in (32, 128):
            g = torch.Generator().manual_seed(7)
            pred_cloud = (torch.rand(b, N, 3, generator=g) * 2 - 1).to(dev).requires_grad_()
            gt_cloud = (torch.rand(b, N, 3, generator=g) * 2 - 1).to(dev)
            with torch.no_grad():
                gt_sil = projection.cont_proj(gt_cloud, H, W, dev, SIGMA_SQ)
            for _ in range(args.trace_steps):
                pred_cloud.grad = None
                proj_loss.get_loss_proj(projection.cont_proj(pred_cloud, H, W, dev, SIGMA_SQ), gt_sil, dev,
                                        'bce_prob')[0].backward()
            torch.cuda.synchronize()
        return
    results = []
    for b in (32, 128):
        g = torch.Generator().manual_seed(7)
        pred_cloud = (torch.rand(b, N, 3, generator=g) * 2 - 1).to(dev).requires_grad_()
        gt_cloud = (torch.rand(b, N, 3, generator=g) * 2 - 1).to(dev)
        with torch.no_grad():
            gt_sil = projection.cont_proj(gt_cloud, H, W, dev, SIGMA_SQ)
        with_torch = b == 32

        def fwd_b():
            with torch.no_grad():
                return projection.cont_proj(pred_cloud, H, W, dev, SIGMA_SQ)

        def step_b():
            pred_cloud.grad = None
            loss = proj_loss.get_loss_proj(projection.cont_proj(pred_cloud, H, W, dev, SIGMA_SQ), gt_sil, dev,
                                           'bce_prob')[0]
            loss.backward()
            return loss.detach()  # nobody keeps the autograd graph (and the cloud's AccumulateGrad node) alive

        def fwd_a():
            with torch.no_grad():
                return torch_cont_proj(pred_cloud, H, W, SIGMA_SQ)

        def step_a():
            pred_cloud.grad = None
            loss = torch_bce_prob(torch_cont_proj(pred_cloud, H, W, SIGMA_SQ), gt_sil)
            loss.backward()
            return loss.detach()

        if with_torch:  # the two sequences agree before anything is timed
            sa, sb = fwd_a(), fwd_b()
            assert torch.allclose(sa, sb, rtol=1e-4, atol=1e-30), float((sa - sb).abs().max())
            la = step_a()
            ga = pred_cloud.grad.clone()
            lb = step_b()
            gb = pred_cloud.grad.clone()
            torch.cuda.synchronize()
            assert abs(la.item() - lb.item()) <= 1e-4 * abs(la.item()) + 1e-6, (la.item(), lb.item())
            scale = float(ga.abs().max())
            assert float((ga - gb).abs().max()) <= 2e-3 * scale, (float((ga - gb).abs().max()), scale)
        reps = 200 if not args.quick else 5
        if with_torch:  # (A) takes milliseconds per call: a quarter of the repetitions fill the window
            reps = max(5, reps // 4)
        fwd = measure({"b": fwd_b, **({"a": fwd_a} if with_torch else {})}, reps, args.rounds)
        step = measure({"b": step_b, **({"a": step_a} if with_torch else {})}, reps, args.rounds)
        floor_us = b * N * H * W / 2.0 / LANE_OPS_PER_S * 1e6
        best_fwd = fwd["b"]["graph_us"] or fwd["b"]["us"]
        row = dict(b=b, n=N, grid_h=H, grid_w=W, sigma_sq=SIGMA_SQ, rounds=args.rounds, forward=fwd, step=step,
                   forward_valu_floor_us=floor_us, forward_share_of_valu_floor=floor_us / best_fwd)
        results.append(row)
        fmt = lambda v: "     n/a" if v is None else f"{v:8.2f}"  # noqa: E731
        print(f"B={b} N={N} {H}x{W} sigma_sq={SIGMA_SQ}", flush=True)
        for what, res in (("forward", fwd), ("step", step)):
            for key, label in (("a", "(A) torch op sequence"), ("b", "(B) silhouette kernels")):
                if key in res:
                    r = res[key]
                    print(f"  {what:7s} {label}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]"
                          f"  graph {fmt(r['graph_us'])} us  kernels/call {r['kernels']}", flush=True)
        print(f"  forward (B): VALU floor {floor_us:.2f} us = {100 * floor_us / best_fwd:.1f} % of {best_fwd:.2f} us",
              flush=True)
    print(json.dumps({"tool": "bench_silhouette", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
