#!/usr/bin/env python3
"""Context.average with and without the fused phase shift against the only way to average a stream without it - torch
index_add_ over the same seven weighted columns (re, im, u, v, w, x, weight) and six divisions - device events, the median
of 20 replays of a captured graph after a warm-up run:
  n5760000    5.76 x 10^6 visibilities (the flagging profile's stream), time-major over 7200 baselines, 8 times per group:
              G = 720000, and the groups of neighbouring samples are neighbouring groups (strided by the baseline count)
  n100000000  10^8 visibilities over 100000 baselines, 10 times per group: G = 10^7
The fused call reads the stream twice where torch reads it seven times; it has to be no slower than the torch composition
(which does not shift at all) at both shapes - the exit status says so - and the measured ratio is what is written down.
Every shape is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/average_timing.py [--reps 20] [--out profiles/average_n5760000.jsonl] [--shapes n5760000,n100000000]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"n5760000": (7200, 800, 8, 300), "n100000000": (100000, 1000, 10, 900)}  # baselines, times, per group, time limit


def step(what, reps):
    import torch
    import gridhip
    from noise_timing import replayed
    B, times, per, _ = SHAPES[what]
    n, G = B * times, B * (times // per)
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    g = torch.Generator(device=dev).manual_seed(4)
    rnd = lambda: torch.randn(n, dtype=torch.float64, device=dev, generator=g)  # noqa: E731
    u, v, w, x = rnd() * 1e3, rnd() * 1e3, rnd() * 10, rnd() * 0.1
    vis = torch.complex(rnd(), rnd())
    wt = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    k = torch.arange(n, dtype=torch.int64, device=dev)
    group = torch.div(torch.div(k, B, rounding_mode="floor"), per, rounding_mode="floor") * B + k % B
    del k
    R = gridhip.rotation_to(0.01, -0.02)
    re, im = vis.real.contiguous(), vis.imag.contiguous()

    def by_torch():
        W = torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, group, wt)
        return [torch.zeros(G, dtype=torch.float64, device=dev).index_add_(0, group, wt * c) / W
                for c in (re, im, u, v, w, x)] + [W]

    base = {"device": torch.cuda.get_device_name(0), "n": n, "G": G, "per_group": per, "shape": what}
    rows = []
    r = replayed(torch, by_torch, lambda: None, reps)
    rows.append(dict(base, what="torch index_add_ x 7 + division", **r))
    t_torch = r["median_ms"]
    for name, rot in (("average", None), ("average, fused shift", R)):
        res = ctx.average((u, v, w), vis, group, G, weights=wt, x=x, R=rot, stats=True)
        r = replayed(torch, lambda: ctx.average((u, v, w), vis, group, G, weights=wt, x=x, R=rot), lambda: None, reps)
        # bytes the two passes read: group, u, v, w, x, re, im, weight = 72 B per visibility and pass
        rows.append(dict(base, what=name, stats=[float(s) for s in res[-1].tolist()], over_torch=r["median_ms"] / t_torch,
                         stream_gb_per_s=2 * 72 * n / r["median_ms"] / 1e6, **r))
    # the averages agree with torch's to rounding (torch's sums are floating-point atomics: not the same bits)
    mine = ctx.average((u, v, w), vis, group, G, weights=wt, x=x)
    ref = by_torch()
    rows[1]["max_rel_diff_to_torch"] = float(((mine[1].real - ref[0]).abs().max() / ref[0].abs().max()).item())
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "average_n5760000.jsonl"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--step", help="run one shape in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(args.step, args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows, shapes = [], [s for s in args.shapes.split(",") if s]
    for what in shapes:
        r = subprocess.run(["timeout", "-k", "10", str(SHAPES[what][3]), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", what], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} ended with status {r.returncode}: nothing more is started", flush=True)
            break
        rows += [json.loads(x) for x in got]
        print("\n".join(got), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    fused = [r for r in rows if r["what"] == "average, fused shift"]
    return 0 if len(fused) == len(shapes) and all(r["over_torch"] <= 1.0 for r in fused) else 1


if __name__ == "__main__":
    sys.exit(main())
