#!/usr/bin/env python3
"""N-D Chamfer distance: chamfer_NDDist (csrc/chamfer_nd.hip) against the torch
composition it replaces and, at D = 3, against chamfer_3DDist, alternated in one
process.

  (N) chamfer_NDDist()(x, y): one pcm_chamfer_nd_forward launch; with the
      backward, one pcm_chamfer_nd_backward launch more.
  (T) the torch composition: torch.cdist(x, y).pow(2), min over each axis, and
      autograd for the backward.  "not measured" where it cannot allocate.
  (3) at D = 3, chamfer_3DDist (the filtered / grid forward, which stays the 3-D
      path).

Shapes: B=32 N=M=1024 and B=8 N=M=16384, D in {2, 3, 6, 8}.  Legs: forward, and
forward + backward of sum(d1) + sum(d2) (which also pays torch's two sums and
autograd's own kernels), and the pcm_chamfer_nd_backward launch alone; (N) and
(3) eager and as a captured graph of GRAPH_CALLS calls, (T) eager. Per leg: device events around `reps`
back-to-back calls (sized for a window of tens of milliseconds) ending in a
synchronise, after a warm-up; `rounds` rounds in which the legs alternate; the
median, the extremes and the spread (max - min) / median are reported.  Also
reported: each (N) time's share of the counted VALU floor -- a pair costs
2 D + 3 lane operations (D subtracts, a multiply, D - 1 fused steps, a compare,
two selects), 2 B N M pairs, 78.6 T lane operations a second.  (N) and (T) are
compared before timing (distances to 1e-4 relative + 1e-6).  The report goes to
stdout and to --out (default profiles/chamfer_nd/bench_chamfer_nd.txt), one JSON
line last; the exit status is 1 if (N) is slower than (T) at the first shape for
any D.

    python tools/bench_chamfer_nd.py [--rounds 5] [--quick] [--dims 2,3,6,8] [--shapes 0,1] [--out PATH]

PCM_HIP_LIB selects another build of the library (make -C csrc variant V=... EXTRA=-DPCM_ND_Q=2: two queries a
lane), which is how the forward's alternatives in DESIGN.md section 3.21 were timed.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "3d-pointcloudreconstruction_amd")
for p in (os.path.join(PKG, "metric"), os.path.join(PKG, "metric", "chamfer3D"), os.path.join(PKG, "metric", "chamferND")):
    if p not in sys.path:
        sys.path.insert(0, p)
import pcm_hip  # noqa: E402
from dist_chamfer_3D import chamfer_3DDist  # noqa: E402
from dist_chamfer_ND import chamfer_NDDist  # noqa: E402

SHAPES = [(32, 1024, 1024), (8, 16384, 16384)]
VALU_FLOOR = 78.6e12  # lane operations per second
GRAPH_CALLS = 2
WINDOW_US = 30000.0  # timed window a leg aims at


def torch_composition(x, y):
    d = torch.cdist(x, y).pow(2)
    d1, i1 = d.min(dim=2)
    d2, i2 = d.min(dim=1)
    return d1, d2, i1, i2


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
    ap.add_argument("--dims", default="2,3,6,8")
    ap.add_argument("--shapes", default="0,1", help="which of the two shapes to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chamfer_nd", "bench_chamfer_nd.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer_nd needs a HIP device")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    report = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    say(f"tile {pcm_hip.CHAMFER_ND_TILE}, {pcm_hip.CHAMFER_ND_QUERIES} queries a workgroup, {pcm_hip.CHAMFER_ND_WAVES} "
        f"waves a tile (library: {pcm_hip.chamfer_nd_geometry()})")
    results = []
    beats = True
    for si, (b, n, m) in enumerate(SHAPES):
        if str(si) not in args.shapes.split(","):
            continue
        for dim in [int(v) for v in args.dims.split(",")]:
            g = torch.Generator().manual_seed(11)
            x = torch.rand(b, n, dim, generator=g).to(dev).requires_grad_()
            y = torch.rand(b, m, dim, generator=g).to(dev).requires_grad_()
            floor_us = 2.0 * b * n * m * (2 * dim + 3) / VALU_FLOOR * 1e6
            nd = chamfer_NDDist()
            c3 = chamfer_3DDist()

            def fwd(fn):
                def run():
                    with torch.no_grad():
                        return fn(x, y)
                return run

            def fwd_bwd(fn):
                def run():
                    x.grad = y.grad = None
                    out = fn(x, y)
                    (out[0].sum() + out[1].sum()).backward()
                return run

            legs = {"nd fwd": fwd(nd), "nd fwd+bwd": fwd_bwd(nd)}
            notes = {}
            # the backward launch alone, on the forward's indices (fwd+bwd also pays torch's sums and autograd)
            with torch.no_grad():
                _, _, i1, i2 = nd(x, y)
            xd, yd = x.detach(), y.detach()
            gd1, gd2 = torch.ones(b, n, device=dev), torch.ones(b, m, device=dev)
            g1, g2 = torch.empty_like(xd), torch.empty_like(yd)
            legs["nd bwd launch"] = lambda: pcm_hip.chamfer_nd_backward(xd, 0, yd, 0, gd1, gd2, i1, i2, g1, g2)
            try:
                want = fwd(torch_composition)()
                got = legs["nd fwd"]()
                torch.cuda.synchronize()
                for a, w in zip(got[:2], want[:2]):
                    assert torch.allclose(a, w, rtol=1e-4, atol=1e-6), float((a - w).abs().max())
                fwd_bwd(torch_composition)()
                torch.cuda.synchronize()
                legs["torch fwd"] = fwd(torch_composition)
                legs["torch fwd+bwd"] = fwd_bwd(torch_composition)
                del want, got
            except torch.OutOfMemoryError as e:
                notes["torch"] = "not measured: " + str(e).split(".")[0]
                torch.cuda.empty_cache()
            if dim == 3:
                legs["3d fwd"] = fwd(c3)
                legs["3d fwd+bwd"] = fwd_bwd(c3)
            graphs = {}
            for k in [k for k in legs if not k.startswith("torch")]:
                try:
                    graphs[k + ", captured"] = captured(legs[k])
                except RuntimeError as e:
                    notes[k + ", captured"] = "not measured: " + str(e).splitlines()[0]
                    torch.cuda.synchronize()
            timed = {}
            for k, fn in legs.items():
                once = eager_us(fn, 1)  # also the warm-up
                once = eager_us(fn, 2)
                reps = 1 if args.quick else max(2, min(2000, int(WINDOW_US / max(once, 1.0))))
                timed[k] = (lambda fn=fn, reps=reps: eager_us(fn, reps))
            for k, gr in graphs.items():
                once = eager_us(gr.replay, 2) / GRAPH_CALLS
                reps = 1 if args.quick else max(1, min(1000, int(WINDOW_US / max(once, 1.0)) // GRAPH_CALLS))
                timed[k] = (lambda gr=gr, reps=reps: eager_us(gr.replay, reps) / GRAPH_CALLS)
            times = {k: [] for k in timed}
            for _ in range(args.rounds):
                for k, leg in timed.items():
                    times[k].append(leg())
            res = {k: stats(v) for k, v in times.items()}
            say(f"B={b} N={n} M={m} D={dim}: counted VALU floor {floor_us:.1f} us")
            for k, v in res.items():
                share = f"  floor / time = {100 * floor_us / v['us']:.1f} %" if k.startswith("nd fwd") else ""
                say(f"  {k:28s} {v['us']:11.1f} us [{v['us_min']:.1f}..{v['us_max']:.1f}] spread {100 * v['spread']:.1f} %{share}")
            for k, v in notes.items():
                say(f"  {k}: {v}")
            row = dict(b=b, n=n, m=m, dim=dim, floor_us=floor_us, legs=res, notes=notes)
            if "torch fwd" in res:
                r_f = res["torch fwd"]["us"] / res["nd fwd"]["us"]
                r_fb = res["torch fwd+bwd"]["us"] / res["nd fwd+bwd"]["us"]
                row["torch_over_nd"] = dict(fwd=r_f, fwd_bwd=r_fb)
                say(f"  (T) / (N) = {r_f:.1f} x forward, {r_fb:.1f} x forward + backward")
                if si == 0 and (r_f < 1.0 or r_fb < 1.0):
                    beats = False
                    say("  -- (N) is SLOWER than the torch composition here")
            if "3d fwd" in res:
                r_f = res["nd fwd"]["us"] / res["3d fwd"]["us"]
                r_fb = res["nd fwd+bwd"]["us"] / res["3d fwd+bwd"]["us"]
                row["nd_over_3d"] = dict(fwd=r_f, fwd_bwd=r_fb)
                say(f"  (N) / (3) = {r_f:.2f} x forward, {r_fb:.2f} x forward + backward")
            results.append(row)
            del graphs, legs, timed
            torch.cuda.empty_cache()
    say(json.dumps({"tool": "bench_chamfer_nd", "device": torch.cuda.get_device_name(0),
                    "beats_torch_at_first_shape": beats, "results": results}))
    report.close()
    return 0 if beats else 1


if __name__ == "__main__":
    sys.exit(main())
