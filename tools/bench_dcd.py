#!/usr/bin/env python3
"""Density-aware Chamfer distance: pcm_dcd_loss against the published loop
written in torch over this project's own chamfer_3DDist, alternated in one
process.

  (A) the published calc_dcd, restated: chamfer_3DDist's forward, exp of both
      distance arrays, then a Python loop over the batch -- bincount, gather,
      pow, add, reciprocal, multiply, multiply, negate-add, mean for each
      direction -- two stacks and the mean; autograd's backward through all of
      it into chamfer_3DDist's backward.  Its bincount reads the largest index
      back to the host, which a capturing stream does not allow, so (A) is
      timed eager only and no capture of it is attempted.
  (B) dcd_loss.calc_dcd: one pcm_dcd_loss call (csrc/dcd.hip): the Chamfer
      forward (one launch, two for the grid forward of large clouds), ONE
      launch for counts, terms, graddists and sums, and the Chamfer backward
      (one launch) when a cloud needs a gradient.

Settings: B=32 N=M=1024 (the flagship shape) and B=8 N=M=16384, alpha = 1000.
Timed per setting and sequence, `forward` (the [B] losses, no gradient) and
`step` (losses, their sum's backward to both clouds):
  us/call   device events around `reps` back-to-back eager calls ending in a
            synchronise, median of `rounds` rounds in which A and B alternate;
  graph us  GRAPH_CALLS back-to-back calls captured once on a single stream
            and replayed, per call ((B) only).
Also the Chamfer forward alone through pcm_hip.chamfer_forward, eager and
captured: the new launch's own time is reported as (B) forward minus it.  The
two sequences' losses and gradients are compared before timing.  The report
goes to stdout and to --out (default profiles/dcd/bench_dcd.txt), one JSON line
last.

    python tools/bench_dcd.py [--rounds 5] [--quick] [--skip-large] [--out PATH]
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
import pcm_hip  # noqa: E402
import dcd_loss  # noqa: E402
from dist_chamfer_3D import chamfer_3DDist  # noqa: E402

SETTINGS = [(32, 1024, 1024), (8, 16384, 16384)]
ALPHA, LAMBDA = 1000.0, 1.0
GRAPH_CALLS = 4
LOOP_OPS = 2 * 9  # torch calls per batch element in (A)'s loop, both directions


def torch_dcd(x, gt, alpha=ALPHA, n_lambda=LAMBDA):
    """[B] losses by the published sequence (its dist1 / idx1 belong to gt's points)."""
    n_x, n_gt = x.shape[1], gt.shape[1]
    frac_12, frac_21 = n_x / n_gt, n_gt / n_x
    dist1, dist2, idx1, idx2 = chamfer_3DDist()(gt, x)
    exp_dist1, exp_dist2 = torch.exp(-dist1 * alpha), torch.exp(-dist2 * alpha)
    loss1, loss2 = [], []
    for b in range(x.shape[0]):
        count1 = torch.bincount(idx1[b])
        weight1 = count1[idx1[b].long()].float().detach() ** n_lambda
        weight1 = (weight1 + 1e-6) ** (-1) * frac_21
        loss1.append((-exp_dist1[b] * weight1 + 1.).mean())
        count2 = torch.bincount(idx2[b])
        weight2 = count2[idx2[b].long()].float().detach() ** n_lambda
        weight2 = (weight2 + 1e-6) ** (-1) * frac_12
        loss2.append((-exp_dist2[b] * weight2 + 1.).mean())
    return (torch.stack(loss1) + torch.stack(loss2)) / 2


def eager_us(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / reps


def captured(fn):
    """A graph of GRAPH_CALLS back-to-back calls on one stream."""
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


def measure(fns, capture, reps, rounds):
    """{name: dict(us, us_min, us_max, graph_us, ..)} with the sequences alternated per round."""
    for _ in range(2):
        for fn in fns.values():
            eager_us(fn, max(2, reps // 4))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(eager_us(fn, reps))
    graphs = {k: captured(fns[k]) for k in capture}
    gtimes = {k: [] for k in fns}
    for _ in range(rounds):
        for k, g in graphs.items():
            gtimes[k].append(eager_us(g.replay, max(2, reps // GRAPH_CALLS)) / GRAPH_CALLS)
    return {k: dict(us=statistics.median(times[k]), us_min=min(times[k]), us_max=max(times[k]),
                    graph_us=statistics.median(gtimes[k]) if gtimes[k] else None,
                    graph_us_min=min(gtimes[k]) if gtimes[k] else None,
                    graph_us_max=max(gtimes[k]) if gtimes[k] else None) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few repetitions (a rehearsal, not a measurement)")
    ap.add_argument("--skip-large", action="store_true", help="leave out B=8 N=M=16384")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dcd", "bench_dcd.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcd needs a HIP device")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    report = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    results = []
    for b, n, m in SETTINGS:
        if args.skip_large and max(n, m) > 4096:
            continue
        g = torch.Generator().manual_seed(7)
        x = torch.rand(b, n, 3, generator=g).to(dev).requires_grad_()
        y = torch.rand(b, m, 3, generator=g).to(dev).requires_grad_()
        xd, yd = x.detach(), y.detach()  # the forward alone: no cloud asks for a gradient
        d1, d2 = torch.empty(b, n, device=dev), torch.empty(b, m, device=dev)
        i1 = torch.empty(b, n, dtype=torch.int32, device=dev)
        i2 = torch.empty(b, m, dtype=torch.int32, device=dev)

        def fwd_b():
            return dcd_loss.calc_dcd(xd, yd, ALPHA, LAMBDA)[0]

        def step_b():
            x.grad = y.grad = None
            loss = dcd_loss.calc_dcd(x, y, ALPHA, LAMBDA)[0]
            loss.sum().backward()
            return loss.detach()

        def fwd_a():
            with torch.no_grad():
                return torch_dcd(xd, yd)

        def step_a():
            x.grad = y.grad = None
            loss = torch_dcd(x, y)
            loss.sum().backward()
            return loss.detach()

        def chamfer_only():
            pcm_hip.chamfer_forward(xd, yd, d1, d2, i1, i2)

        la = step_a()  # the two sequences agree before anything is timed
        ga = (x.grad.clone(), y.grad.clone())
        lb = step_b()
        gb = (x.grad.clone(), y.grad.clone())
        torch.cuda.synchronize()
        assert torch.allclose(la, lb, rtol=1e-4, atol=1e-6), float((la - lb).abs().max())
        assert torch.allclose(fwd_a(), fwd_b(), rtol=1e-4, atol=1e-6)
        for u, v in zip(ga, gb):
            assert float((u - v).abs().max()) <= 1e-4 * float(u.abs().max()) + 1e-9, float((u - v).abs().max())
        reps = 3 if args.quick else (20 if n * m <= 1 << 20 else 5)
        fwd = measure({"b": fwd_b, "a": fwd_a, "chamfer": chamfer_only}, ("b", "chamfer"), reps, args.rounds)
        step = measure({"b": step_b, "a": step_a}, ("b",), reps, args.rounds)
        grid = pcm_hip.load_library().pcm_chamfer_forward_ws_bytes(b, n, m) > 0
        launches = dict(forward=(2 if grid else 1) + 1, step=(2 if grid else 1) + 2)
        results.append(dict(b=b, n=n, m=m, alpha=ALPHA, n_lambda=LAMBDA, rounds=args.rounds, launches=launches,
                            loss_mean=float(lb.mean()), forward=fwd, step=step))
        fmt = lambda v: "      n/a" if v is None else f"{v:9.2f}"  # noqa: E731
        say(f"B={b} N={n} M={m} alpha={ALPHA:g} lambda={LAMBDA:g}: mean loss {float(lb.mean()):.4f}; (B) launches "
            f"{launches['forward']} a loss-only call ({'grid' if grid else 'dense'} forward + the terms launch), "
            f"{launches['step']} with gradients, plus autograd's two multiplies in a step; (A) {LOOP_OPS} torch calls "
            f"a batch element = {LOOP_OPS * b} in its loop, beside the forward, two exp, two stack and the mean")
        for what, res in (("forward", fwd), ("step", step)):
            for key, label in (("a", "(A) published loop in torch"), ("b", "(B) pcm_dcd_loss")):
                r = res[key]
                say(f"  {what:7s} {label}: {fmt(r['us'])} us/call [{r['us_min']:.2f}..{r['us_max']:.2f}]"
                    f"  graph {fmt(r['graph_us'])} us")
            best = res["b"]["graph_us"]
            say(f"  {what:7s} (A) eager / (B) eager = {res['a']['us'] / res['b']['us']:.1f} x; (A) eager / (B) graph = "
                f"{res['a']['us'] / best:.1f} x" + ("" if res["a"]["us"] > res["b"]["us"]
                                                    else "  -- (B) is NOT faster than the torch loop here"))
        c = fwd["chamfer"]
        say(f"  Chamfer forward alone: {fmt(c['us'])} us/call eager, graph {fmt(c['graph_us'])} us; the terms launch = "
            f"(B) forward - it = {fwd['b']['graph_us'] - c['graph_us']:.2f} us captured "
            f"({100 * (fwd['b']['graph_us'] - c['graph_us']) / c['graph_us']:.0f} % of the forward), "
            f"{fwd['b']['us'] - c['us']:.2f} us eager (with calc_dcd's Python and two allocations)")
    say(json.dumps({"tool": "bench_dcd", "device": torch.cuda.get_device_name(0), "results": results}))
    report.close()


if __name__ == "__main__":
    main()
