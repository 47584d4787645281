#!/usr/bin/env python3
"""Farthest point sampling: the one-launch kernel against a torch restatement
of the reference's loop, alternated in one process.

  (A) the reference's loop on the device, restated here: per iteration the
      centroid gather, the broadcast difference, its square and sum, the
      compare, the boolean-mask assignment (which synchronises with the host)
      and the row-wise argmax (utils/utils.py:353-359), then index_points'
      gather (:316-332) -- what utils/datasets_sample_pcl.py:87-94 runs;
  (B) sampling.sample_points: pcm_fps (csrc/sampling.hip), indices and points
      from one launch -- with the workgroup size the library picks for N, and
      with every size that holds the cloud forced (64, 256, 1024 threads).

Shapes: B=32, N=1024, S=128 and S=256 (the reference's two calls at a training
batch) and B=8, N=16384, S=1024.  Per shape and sequence:
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise, median of `rounds` rounds in which the sequences
            alternate (every sequence warmed at the timed shape first);
  graph us  ten back-to-back calls captured once and replayed, per call (a
            replay's own fixed cost is shared by the ten); (A) cannot be
            captured: its mask assignment reads the device;
  ns/iter   the time per call (graph if there is one) divided by S -- with
            B clouds on B compute units at once, the latency of one
            iteration's chain;
  kernels   device kernels per call, counted by torch.profiler in an untimed pass.
Both sequences' indices are compared before timing.  One JSON line at the end.

    python tools/bench_fps.py [--rounds 5] [--quick] [--sweep]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "utils")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcm_hip  # noqa: E402
import sampling  # noqa: E402

SHAPES = [(32, 1024, 128), (32, 1024, 256), (8, 16384, 1024)]  # (B, N, S)


def torch_fps(xyz, npoint, start):
    """Sequence (A): farthest point sampling as a loop of torch operations with
    the same per-iteration work as the reference's -- an indexed gather of the
    current point, a broadcast squared distance, a compare, a masked overwrite
    of the running minima (boolean indexing: the host waits for the mask's
    count) and a row-wise argmax -- followed by one gather of the chosen points."""
    b, n, _ = xyz.shape
    dev = xyz.device
    batch = torch.arange(b, device=dev)
    chosen = torch.empty(b, npoint, dtype=torch.long, device=dev)
    gap = torch.full((b, n), 1e10, dtype=xyz.dtype, device=dev)  # squared distance to the nearest chosen point
    current = torch.full((b,), start, dtype=torch.long, device=dev)
    for step in range(npoint):
        chosen[:, step] = current
        pivot = xyz[batch, current].unsqueeze(1)
        sq = (xyz - pivot).pow(2).sum(-1)
        shrink = sq < gap
        gap[shrink] = sq[shrink]
        current = gap.argmax(-1)
    return chosen, xyz[batch.unsqueeze(1), chosen]


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
    """A graph of GRAPH_CALLS back-to-back calls."""
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


def kernels_per_call(fn, calls=2):
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


def measure(fns, reps, rounds, capturable):
    """{name: dict(us, us_min, us_max, graph_us, kernels)} with the sequences alternated per round."""
    for _ in range(2):  # warm-up of every sequence at the timed shape
        for k, fn in fns.items():
            eager_us(fn, max(1, reps[k] // 4))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(eager_us(fn, reps[k]))
    graphs = {k: captured(fn) for k, fn in fns.items() if k in capturable}
    gtimes = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            gtimes[k].append(eager_us(g.replay, max(2, reps[k] // GRAPH_CALLS)) / GRAPH_CALLS)
    out = {}
    for k, fn in fns.items():
        gt = gtimes.get(k)
        out[k] = dict(us=statistics.median(times[k]), us_min=min(times[k]), us_max=max(times[k]),
                      graph_us=statistics.median(gt) if gt else None, graph_us_min=min(gt) if gt else None,
                      graph_us_max=max(gt) if gt else None, kernels=kernels_per_call(fn))
    return out


SWEEP_N = [64, 65, 128, 256, 512, 1024, 2048, 4096, 8192, 8193, 16384]
SWEEP_B, SWEEP_S = 32, 128


def sweep(dev, rounds, reps):
    """The workgroup-size table: ns per iteration of every size that holds the
    cloud, by n, as captured graphs (B=32 clouds on 32 compute units, S=128);
    the sizes alternate inside a round.  Where the library's choice
    (csrc/sampling.hip fps_default_threads) comes from."""
    rows = []
    print(f"ns per iteration, B={SWEEP_B} S={SWEEP_S}, graph replay, median of {rounds} rounds", flush=True)
    print("      n " + "".join(f"{t:>9d}" for t in pcm_hip.FPS_THREADS) + "   library picks", flush=True)
    for n in SWEEP_N:
        g = torch.Generator().manual_seed(7)
        xyz = torch.rand(SWEEP_B, n, 3, generator=g).to(dev)
        idx = torch.empty(SWEEP_B, SWEEP_S, dtype=torch.long, device=dev)
        pts = torch.empty(SWEEP_B, SWEEP_S, 3, device=dev)
        graphs = {}
        for t in pcm_hip.FPS_THREADS:
            def fn(t=t):
                pcm_hip.fps(xyz, 0, SWEEP_S, 0, idx, pts, threads=t)
            try:
                fn()
            except pcm_hip.PcmError:  # the size cannot hold the cloud: rejected on the host
                continue
            graphs[t] = captured(fn)
        times = {t: [] for t in graphs}
        for r in range(rounds + 1):  # the first round warms up
            for t, gr in graphs.items():
                us = eager_us(gr.replay, max(2, reps // GRAPH_CALLS)) / GRAPH_CALLS
                if r:
                    times[t].append(us)
        ns = {t: statistics.median(v) * 1000.0 / SWEEP_S for t, v in times.items()}
        pick = pcm_hip.fps_default_threads(n)
        rows.append(dict(n=n, ns_per_iteration={str(t): v for t, v in ns.items()}, default_threads=pick,
                         fastest=min(ns, key=ns.get)))
        print(f"{n:7d} " + "".join(f"{ns[t]:9.1f}" if t in ns else "        -" for t in pcm_hip.FPS_THREADS)
              + f"   {pick}", flush=True)
    print(json.dumps({"tool": "bench_fps --sweep", "device": torch.cuda.get_device_name(0), "b": SWEEP_B,
                      "npoint": SWEEP_S, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true",
                    help="only the workgroup-size table: every size that holds the cloud, by n")
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fps needs a HIP device")
    dev = torch.device("cuda:0")
    if args.sweep:
        sweep(dev, args.rounds, 200 if not args.quick else 20)
        return
    results = []
    for b, n, s in SHAPES:
        g = torch.Generator().manual_seed(7)
        xyz = torch.rand(b, n, 3, generator=g).to(dev)
        idx = torch.empty(b, s, dtype=torch.long, device=dev)
        pts = torch.empty(b, s, 3, device=dev)

        def seq_a():
            return torch_fps(xyz, s, 0)

        def forced(threads):
            return lambda: pcm_hip.fps(xyz, 0, s, 0, idx, pts, threads=threads)

        fns = {"a": seq_a, "b": lambda: sampling.sample_points(xyz, s)}
        # a size that cannot hold the cloud is rejected on the host (PcmError)
        for t in pcm_hip.FPS_THREADS:
            try:
                forced(t)()
                fns[f"b{t}"] = forced(t)
            except pcm_hip.PcmError:
                pass
        torch.cuda.synchronize()

        # the sequences agree before anything is timed (rows where the torch sum's
        # last bits decide a near-tie aside: counted, not hidden)
        ia, pa = seq_a()
        ib, pb = sampling.sample_points(xyz, s)
        same_rows = int((ia == ib).all(1).sum())
        for k in fns:
            if k.startswith("b") and k != "b":
                fns[k]()
                assert torch.equal(idx, ib) and torch.equal(pts, pb), k
        assert torch.equal(pb, xyz[torch.arange(b, device=dev).view(b, 1), ib])
        torch.cuda.synchronize()

        ours = 100 if not args.quick else 3
        theirs = 3 if not args.quick else 1
        if s >= 1024:
            ours, theirs = max(3, ours // 4), max(1, theirs // 3)
        reps = {k: (theirs if k == "a" else ours) for k in fns}
        res = measure(fns, reps, args.rounds, capturable=[k for k in fns if k != "a"])
        for r in res.values():
            best = r["graph_us"] or r["us"]
            r["ns_per_iteration"] = best * 1000.0 / s
        default_threads = pcm_hip.fps_default_threads(n)
        row = dict(b=b, n=n, npoint=s, rounds=args.rounds, default_threads=default_threads,
                   rows_equal_to_torch=same_rows, sequences=res,
                   speedup_eager=res["a"]["us"] / res["b"]["us"])
        results.append(row)
        fmt = lambda v: "      n/a" if v is None else f"{v:9.2f}"  # noqa: E731
        print(f"B={b} N={n} S={s}  (library picks {default_threads} threads; {same_rows}/{b} rows equal to torch's)",
              flush=True)
        for key, r in res.items():
            label = {"a": "(A) torch loop", "b": "(B) sample_points"}.get(key, f"    pcm_fps, {key[1:]} threads")
            print(f"  {label:24s}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]  graph "
                  f"{fmt(r['graph_us'])} us  {r['ns_per_iteration']:9.1f} ns/iter  kernels/call {r['kernels']}",
                  flush=True)
        print(f"  (A) / (B) eager: {row['speedup_eager']:.0f}x", flush=True)
    print(json.dumps({"tool": "bench_fps", "device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()
