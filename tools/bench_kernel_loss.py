#!/usr/bin/env python3
"""Kernel-norm (MMD) loss: pcm_kernel_loss against a torch restatement of the
same formula, alternated in one process.

  (A) the formula in torch on the device: the three broadcast difference
      tensors [B, N, N, 3], [B, M, M, 3] and [B, N, M, 3], their squared norms,
      exp, the weighted sums, and autograd's backward to both clouds (what a
      dense geomloss-style implementation does).
  (B) kernel_loss.SamplesLoss('gaussian', blur=0.2): one pcm_kernel_loss call
      (csrc/kernel_loss.hip), the gradients from the same scan.

Settings: B=32 N=M=1024; B=32 N=256 M=1024; B=8 N=M=16384 ((B) only: (A)'s
tensors would take 77 GiB each).  Timed per setting and sequence, `forward`
(the [B] losses, no gradient) and `step` (losses, their sum's backward to both
clouds):
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise, median of `rounds` rounds in which A and B alternate;
  graph us  ten back-to-back calls captured once on a single stream and
            replayed, per call;
and for (B) the time against the counted VALU floor: B (N + M)^2 pairs at 12
issue slots a pair with gradients (3 subtractions, 3 for the squared distance,
the scale, 2 for the exp2, 4 accumulates) and 9 without, over 78.6 T lane-op/s.
The two sequences' losses and gradients are compared before timing.  The report
goes to stdout and to --out (default profiles/kernel_loss/bench_kernel_loss.txt),
one JSON line last.

    python tools/bench_kernel_loss.py [--rounds 5] [--quick] [--out PATH]
    rocprofv3 --kernel-trace --stats -- python tools/bench_kernel_loss.py --trace-steps 30
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "loss")):
    if p not in sys.path:
        sys.path.insert(0, p)
import kernel_loss  # noqa: E402

LANE_OPS_PER_S = 78.6e12  # fp32 VALU lane operations per second
SLOTS_STEP, SLOTS_FORWARD = 12, 9
BLUR = 0.2
SETTINGS = [(32, 1024, 1024, True), (32, 256, 1024, True), (8, 16384, 16384, False)]
GRAPH_CALLS = 10


def torch_gaussian(x, y, blur):
    """[B] kernel norms from the three broadcast difference tensors."""
    def k(p, q):
        diff = p[:, :, None, :] - q[:, None, :, :]
        return torch.exp(-(diff * diff).sum(-1) / (2 * blur * blur))
    n, m = x.shape[1], y.shape[1]
    return (0.5 * k(x, x).sum((1, 2)) / (n * n) + 0.5 * k(y, y).sum((1, 2)) / (m * m)
            - k(x, y).sum((1, 2)) / (n * m))


def eager_us(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / reps


def captured(fn):
    """A graph of GRAPH_CALLS back-to-back calls on one stream, or None where the sequence cannot be captured."""
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


def measure(fns, reps, rounds):
    """{name: dict(us, us_min, us_max, graph_us, ..)} with the sequences alternated per round."""
    for _ in range(2):
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
    return {k: dict(us=statistics.median(times[k]), us_min=min(times[k]), us_max=max(times[k]),
                    graph_us=statistics.median(gtimes[k]) if gtimes[k] else None,
                    graph_us_min=min(gtimes[k]) if gtimes[k] else None,
                    graph_us_max=max(gtimes[k]) if gtimes[k] else None) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kernel_loss", "bench_kernel_loss.txt"))
    ap.add_argument("--trace-steps", type=int, default=0,
                    help="only run this many eager (B) steps at B=32, N=M=1024, untimed: the workload for a "
                         "kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kernel_loss needs a HIP device")
    dev = torch.device("cuda:0")
    if args.trace_steps:
        g = torch.Generator().manual_seed(7)
        x = torch.rand(32, 1024, 3, generator=g).to(dev).requires_grad_()
        y = (torch.rand(32, 1024, 3, generator=g) * 0.25 + 0.75).to(dev).requires_grad_()
        L = kernel_loss.SamplesLoss("gaussian", blur=BLUR)
        for _ in range(args.trace_steps):
            x.grad = y.grad = None
            L(x, y).sum().backward()
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    report = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    L = kernel_loss.SamplesLoss("gaussian", blur=BLUR)
    results = []
    for b, n, m, with_torch in SETTINGS:
        g = torch.Generator().manual_seed(7)
        x = torch.rand(b, n, 3, generator=g).to(dev).requires_grad_()
        y = (torch.rand(b, m, 3, generator=g) * 0.25 + 0.75).to(dev).requires_grad_()

        xd, yd = x.detach(), y.detach()  # the forward alone: no cloud asks for a gradient

        def fwd_b():
            return L(xd, yd)

        def step_b():
            x.grad = y.grad = None
            loss = L(x, y)
            loss.sum().backward()
            return loss.detach()

        def fwd_a():
            return torch_gaussian(xd, yd, BLUR)

        def step_a():
            x.grad = y.grad = None
            loss = torch_gaussian(x, y, BLUR)
            loss.sum().backward()
            return loss.detach()

        if with_torch:  # the two sequences agree before anything is timed
            la = step_a()
            ga = (x.grad.clone(), y.grad.clone())
            lb = step_b()
            gb = (x.grad.clone(), y.grad.clone())
            torch.cuda.synchronize()
            assert torch.allclose(la, lb, rtol=1e-4, atol=1e-6), float((la - lb).abs().max())
            assert torch.allclose(fwd_a(), fwd_b(), rtol=1e-4, atol=1e-6)
            for u, v in zip(ga, gb):
                assert float((u - v).abs().max()) <= 1e-3 * float(u.abs().max()), float((u - v).abs().max())
        reps = 5 if args.quick else (100 if n * m <= 1 << 20 else 10)
        fns_f = {"b": fwd_b, **({"a": fwd_a} if with_torch else {})}
        fns_s = {"b": step_b, **({"a": step_a} if with_torch else {})}
        fwd = measure(fns_f, reps, args.rounds)
        step = measure(fns_s, reps, args.rounds)
        pairs = b * (n + m) ** 2
        floors = dict(forward=pairs * SLOTS_FORWARD / LANE_OPS_PER_S * 1e6, step=pairs * SLOTS_STEP / LANE_OPS_PER_S * 1e6)
        results.append(dict(b=b, n=n, m=m, blur=BLUR, rounds=args.rounds, pairs=pairs, forward=fwd, step=step,
                            valu_floor_us=floors))
        fmt = lambda v: "     n/a" if v is None else f"{v:9.2f}"  # noqa: E731
        say(f"B={b} N={n} M={m} gaussian blur={BLUR}: {pairs / 1e6:.0f} M pairs")
        for what, res in (("forward", fwd), ("step", step)):
            for key, label in (("a", "(A) torch broadcast"), ("b", "(B) pcm_kernel_loss")):
                if key in res:
                    r = res[key]
                    say(f"  {what:7s} {label}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]"
                        f"  graph {fmt(r['graph_us'])} us")
            best = res["b"]["graph_us"] or res["b"]["us"]
            line = f"  {what:7s} (B): counted VALU floor {floors[what]:.2f} us = {100 * floors[what] / best:.1f} % of {best:.2f} us"
            if "a" in res:
                line += f"; (A) / (B) = {(res['a']['graph_us'] or res['a']['us']) / best:.1f} x"
            say(line)
    say(json.dumps({"tool": "bench_kernel_loss", "device": torch.cuda.get_device_name(0), "results": results}))
    report.close()


if __name__ == "__main__":
    main()
