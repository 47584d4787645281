#!/usr/bin/env python3
"""Cross Chamfer matrix: pcm_chamfer_cross against the two other ways to the
same [S, R] matrices, alternated in one process.

  (N) cross_chamfer_3D.chamfer_cross(x, y): one pcm_chamfer_cross call
      (csrc/chamfer_cross.hip) -- the scan of both directions and, for clouds
      of more than 1024 points, a finalise launch.  Timed eager and captured.
  (A) what the library offered before: a loop over the R gallery clouds of
      chamfer_3DEval on y[j] expanded to S copies (R calls of two launches
      each, R copies of S x M points), its mean distances gathered into the
      matrices.
  (B) a float64 broadcast formulation in torch: the [ci, cj, N, M, 3]
      differences of a chunk of cloud pairs, squared, summed, two min
      reductions and two means, chunked to CHUNK_ELEMS distances at a time.
      Where the whole matrix would take seconds it is timed on the first
      `B_ROWS` query clouds against the whole gallery and scaled by S / B_ROWS
      (marked "scaled"); the chunks are independent, so the scaling is exact up
      to the last partial chunk.

Shapes: retrieval S=32 R=1024 N=M=1024; set metrics S=R=256 N=M=2048; small
S=R=32 N=M=1024.  Per shape and leg: device events around `reps` back-to-back
calls ending in a synchronise, after a warm-up; `rounds` rounds in which the
legs alternate; the median, the extremes and the spread (max - min) / median of
each leg are reported.  (N) is NOT slower than (A) when its median does not
exceed (A)'s by more than the larger of the two spreads.  Also reported: distance
evaluations per second (2 S R N M: both directions) and the share of the counted
VALU floor as DESIGN.md section 3.11 counts it -- the scan's 7 packed-fp32
instructions a pair of candidates at 32 lanes a cycle and SIMD, 78.6 T
lane-ops/s / 7 = 11.23 T evaluations/s.  (N) and (A) are compared entry by entry
before timing ((A) adds in float32: 1e-4 relative), (N) and (B) to 1e-6.  The
report goes to stdout and to --out (default profiles/cross/bench_cross.txt), one
JSON line last; the exit status is 1 if (N) is slower than (A) at any shape.

    python tools/bench_cross.py [--rounds 5] [--quick] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "metric", "chamfer3D")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcm_hip  # noqa: E402
from cross_chamfer_3D import chamfer_cross  # noqa: E402
from eval_chamfer_3D import chamfer_3DEval  # noqa: E402

SETTINGS = [("retrieval", 32, 1024, 1024, 1024), ("set metrics", 256, 256, 2048, 2048), ("small", 32, 32, 1024, 1024)]
VALU_FLOOR = 78.6e12  # lane operations per second
LANE_OPS = 7  # per distance evaluation at that rate (the floor is 11.23 T evaluations/s)
CHUNK_ELEMS = 1 << 25  # distances per chunk of (B): 0.8 GB of float64 differences
B_ROWS = 4  # query clouds (B) is timed on where the whole matrix is too slow
B_FULL_MAX = 1 << 32  # distance evaluations up to which (B) runs the whole matrix
GRAPH_CALLS = 2


def loop_eval(x, y):
    """(A): mean12, mean21 [S, R] by R chamfer_3DEval calls on expanded gallery clouds."""
    s, r = x.shape[0], y.shape[0]
    ev = chamfer_3DEval((1e-4,))
    m12 = torch.empty(s, r, device=x.device)
    m21 = torch.empty(s, r, device=x.device)
    for j in range(r):
        res = ev(x, y[j:j + 1].expand(s, -1, -1))
        m12[:, j] = res.mean_dist1
        m21[:, j] = res.mean_dist2
    return m12, m21


def broadcast_f64(x, y, rows=None):
    """(B): mean12, mean21 [rows or S, R] in float64."""
    xs = x[:rows] if rows else x
    s, n = xs.shape[:2]
    r, m = y.shape[:2]
    cj = max(1, min(r, CHUNK_ELEMS // (n * m)))
    x64, y64 = xs.double(), y.double()
    m12 = torch.empty(s, r, dtype=torch.float64, device=x.device)
    m21 = torch.empty(s, r, dtype=torch.float64, device=x.device)
    for i in range(s):
        for j in range(0, r, cj):
            d = (x64[i, None, :, None, :] - y64[j:j + cj, None, :, :]).pow(2).sum(-1)  # [cj, N, M]
            m12[i, j:j + cj] = d.min(dim=2).values.mean(dim=1)
            m21[i, j:j + cj] = d.min(dim=1).values.mean(dim=1)
    return m12, m21


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
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def stats(times):
    med = statistics.median(times)
    return dict(us=med, us_min=min(times), us_max=max(times), spread=(max(times) - min(times)) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one repetition a leg (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cross", "bench_cross.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross needs a HIP device")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    report = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    results = []
    all_ok = True
    for name, s, r, n, m in SETTINGS:
        g = torch.Generator().manual_seed(11)
        x = torch.rand(s, n, 3, generator=g).to(dev)
        y = torch.rand(r, m, 3, generator=g).to(dev)
        evals = 2.0 * s * r * n * m
        full_b = evals <= B_FULL_MAX
        rows = None if full_b else B_ROWS
        scale = 1.0 if full_b else s / B_ROWS

        def new():
            return chamfer_cross(x, y)

        def loop():
            return loop_eval(x, y)

        def bcast():
            return broadcast_f64(x, y, rows)

        got = new()
        a12, a21 = loop()
        b12, b21 = bcast()
        torch.cuda.synchronize()
        nb = b12.shape[0]
        err_a = max(float(((got.mean12 - a12).abs() / a12).max()), float(((got.mean21 - a21).abs() / a21).max()))
        err_b = max(float(((got.mean12[:nb].double() - b12).abs() / b12).max()),
                    float(((got.mean21[:nb].double() - b21).abs() / b21).max()))
        assert err_a <= 1e-4 and err_b <= 1e-6, (err_a, err_b)

        reps_new = 1 if args.quick else (20 if evals < 1e10 else 4)
        graph = captured(new)
        legs = {"new": lambda: eager_us(new, reps_new),
                "graph": lambda: eager_us(graph.replay, max(1, reps_new // GRAPH_CALLS)) / GRAPH_CALLS,
                "loop": lambda: eager_us(loop, 1)}
        times = {k: [] for k in legs}
        for leg in legs.values():  # warm-up
            leg()
        for _ in range(args.rounds):
            for k, leg in legs.items():
                times[k].append(leg())
        tb = [eager_us(bcast, 1) * scale for _ in range(1 if args.quick else 2)]
        res = {k: stats(v) for k, v in times.items()}
        res["bcast"] = stats(tb)
        best = min(res["new"]["us"], res["graph"]["us"])
        slack = max(res["new"]["spread"], res["loop"]["spread"]) * res["loop"]["us"]
        ok = res["new"]["us"] <= res["loop"]["us"] + slack
        all_ok = all_ok and ok
        rate = evals / (res["new"]["us"] * 1e-6)
        share = rate * LANE_OPS / VALU_FLOOR
        run = pcm_hip.chamfer_cross_run(s, r, n, m)
        results.append(dict(name=name, s=s, r=r, n=n, m=m, run=run, evals=evals, rel_err_loop=err_a, rel_err_bcast=err_b,
                            bcast_scaled_from_rows=rows, legs=res, evals_per_s=rate, valu_floor_share=share,
                            not_slower_than_loop=ok))
        say(f"{name}: S={s} R={r} N={n} M={m}; {evals:.3g} distance evaluations; runs of {run} target clouds; "
            f"largest relative difference to (A) {err_a:.2g}, to (B) {err_b:.2g}")
        for key, label in (("new", "(N) pcm_chamfer_cross, eager"), ("graph", "(N) pcm_chamfer_cross, captured"),
                           ("loop", f"(A) {r} chamfer_3DEval calls"),
                           ("bcast", "(B) float64 broadcast" + ("" if full_b else f", scaled from {B_ROWS} of {s} rows"))):
            v = res[key]
            say(f"  {label:52s} {v['us']:12.1f} us [{v['us_min']:.1f}..{v['us_max']:.1f}] spread {100 * v['spread']:.1f} %")
        say(f"  (A) / (N) = {res['loop']['us'] / res['new']['us']:.2f} x eager, {res['loop']['us'] / best:.2f} x best; "
            f"(B) / (N) = {res['bcast']['us'] / res['new']['us']:.1f} x; {rate:.3g} evaluations/s = "
            f"{100 * share:.1f} % of the counted VALU floor"
            + ("" if ok else "  -- (N) is SLOWER than the loop over the existing kernel here"))
    say(json.dumps({"tool": "bench_cross", "device": torch.cuda.get_device_name(0), "not_slower_than_loop": all_ok,
                    "results": results}))
    report.close()
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
