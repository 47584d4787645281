#!/usr/bin/env python3
"""F-score evaluation: the sequence available before pcm_chamfer_eval against
the one-pass path, alternated in one process.

  (A) chamfer_3DDist (argmin forward, four per-point arrays) and then, per
      threshold, the torch ops of the reference's loss/loss_.py:132-138
      (compare, cast, mean, mean, arithmetic, NaN fix-up, three batch means);
  (B) loss_.fscore for one threshold, eval_chamfer_3D.chamfer_eval_batch for
      several: one pcm_chamfer_eval call whatever the number of thresholds.

Shapes: B=32, N=M=1024 float32 (BASELINE config 2) and B=8, N=M=16384 float16
(config 5), each with 1 and 3 thresholds.  Per setting and sequence:
  us/call   device events around `reps` back-to-back eager calls (what a
            caller's evaluation loop pays, launch gaps included), median of
            `rounds` rounds in which A and B alternate;
  graph us  the same calls captured once and replayed (device time without the
            host's enqueue cost), where the sequence can be captured;
  kernels   device kernels per call, counted by torch.profiler in an untimed pass;
and for (B) the pairs/s (2 B N M distance evaluations per call) against the
ceiling of 7 lane operations per pair, 78.6 T lane-op/s / 7.
Both sequences' F-scores are compared before timing.  One JSON line at the end.

    python tools/bench_fscore.py [--rounds 7] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "metric", "chamfer3D"), os.path.join(PKG, "loss")):
    if p not in sys.path:
        sys.path.insert(0, p)
import dist_chamfer_3D  # noqa: E402
import eval_chamfer_3D  # noqa: E402
import loss_  # noqa: E402

LANE_OPS_PER_S = 78.6e12  # packed-fp32 VALU lane operations per second
OPS_PER_PAIR = 7
THRESHOLDS = (1e-4, 2.5e-4, 1e-3)


def sequence_a(x, y, ths):
    """The parent commit's route: the forward, then loss_.py:132-138 per threshold."""
    d1, d2, _, _ = dist_chamfer_3D.chamfer_3DDist()(x, y)
    dist1, dist2 = d2, d1  # the reference's naming: dist1 is per point of Y
    out = []
    for th in ths:
        precision_1 = torch.mean((dist1 < th).float(), dim=1)
        precision_2 = torch.mean((dist2 < th).float(), dim=1)
        fscore = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
        fscore[torch.isnan(fscore)] = 0
        out.append((torch.mean(fscore), torch.mean(precision_1), torch.mean(precision_2)))
    return out


def sequence_b(x, y, ths):
    if len(ths) == 1:
        return [loss_.fscore(x, y, ths[0])]
    _, batch = eval_chamfer_3D.chamfer_eval_batch(x, y, ths)
    return [(batch[t, 0], batch[t, 2], batch[t, 1]) for t in range(len(ths))]


def eager_us(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / reps


def captured(fn):
    """A graph of one call, or None where the sequence cannot be captured."""
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return g
    except Exception as e:  # noqa: BLE001 (a sequence with a host read cannot be captured)
        print(f"    (not capturable: {type(e).__name__})", flush=True)
        torch.cuda.synchronize()
        return None


def kernels_per_call(fn, calls=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fscore needs a HIP device")
    dev = torch.device("cuda:0")
    results = []
    for (b, n, m, dtype, reps) in ((32, 1024, 1024, torch.float32, 200), (8, 16384, 16384, torch.float16, 20)):
        if args.quick:
            reps = max(2, reps // 10)
        g = torch.Generator().manual_seed(5)
        # a prediction scattered around its ground truth: the regime the metric is used in
        y = torch.rand(b, m, 3, generator=g)
        pick = torch.randint(0, m, (b, n), generator=g)
        x = torch.gather(y, 1, pick[:, :, None].expand(b, n, 3)) + 0.01 * torch.randn(b, n, 3, generator=g)
        x, y = x.to(dev, dtype).contiguous(), y.to(dev, dtype).contiguous()
        for nth in (1, 3):
            ths = THRESHOLDS[:nth]
            fa = lambda: sequence_a(x, y, ths)  # noqa: E731
            fb = lambda: sequence_b(x, y, ths)  # noqa: E731
            ra, rb = fa(), fb()
            torch.cuda.synchronize()
            for (a3, b3) in zip(ra, rb):
                for va, vb in zip(a3, b3):
                    # (A)'s torch means sum 32 terms in another order: a few ulp apart
                    assert abs(va.item() - vb.item()) <= 1e-5 * abs(va.item()), (va.item(), vb.item())
            for _ in range(3):  # warm-up
                eager_us(fa, reps)
                eager_us(fb, reps)
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(eager_us(fa, reps))
                tb.append(eager_us(fb, reps))
            ga, gb = captured(fa), captured(fb)
            tga, tgb = [], []
            for _ in range(args.rounds):
                if ga is not None:
                    tga.append(eager_us(ga.replay, reps))
                if gb is not None:
                    tgb.append(eager_us(gb.replay, reps))
            ka, kb = kernels_per_call(fa), kernels_per_call(fb)
            med = lambda v: statistics.median(v) if v else None  # noqa: E731
            row = dict(b=b, n=n, m=m, dtype=str(dtype).replace("torch.", ""), thresholds=nth, reps=reps,
                       rounds=args.rounds,
                       a_us=med(ta), a_us_min=min(ta), a_us_max=max(ta), a_graph_us=med(tga), a_kernels=ka,
                       b_us=med(tb), b_us_min=min(tb), b_us_max=max(tb), b_graph_us=med(tgb), b_kernels=kb)
            best_b = row["b_graph_us"] or row["b_us"]
            row["b_pairs_per_s"] = 2.0 * b * n * m / (best_b * 1e-6)
            row["b_share_of_7op_ceiling"] = row["b_pairs_per_s"] / (LANE_OPS_PER_S / OPS_PER_PAIR)
            results.append(row)
            fmt = lambda v: "   n/a" if v is None else f"{v:8.2f}"  # noqa: E731
            print(f"B={b} N={n} M={m} {row['dtype']} thresholds={nth}", flush=True)
            print(f"  (A) forward + torch ops : {fmt(row['a_us'])} us/call [{row['a_us_min']:.2f}..{row['a_us_max']:.2f}]"
                  f"  graph {fmt(row['a_graph_us'])} us  kernels/call {ka}", flush=True)
            print(f"  (B) pcm_chamfer_eval    : {fmt(row['b_us'])} us/call [{row['b_us_min']:.2f}..{row['b_us_max']:.2f}]"
                  f"  graph {fmt(row['b_graph_us'])} us  kernels/call {kb}", flush=True)
            print(f"  (B) {row['b_pairs_per_s'] / 1e12:.3f} T pairs/s = "
                  f"{100 * row['b_share_of_7op_ceiling']:.1f} % of the {LANE_OPS_PER_S / OPS_PER_PAIR / 1e12:.2f} T "
                  "pairs/s 7-lane-op ceiling", flush=True)
    print(json.dumps({"tool": "bench_fscore", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
