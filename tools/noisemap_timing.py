#!/usr/bin/env python3
"""Context.noise_map at N = 2400 (the driver's image size) on one device, device events around windows of calls:
  nodes     the node table alone (maps=False, mode None) for (step, half) = (16, 32) and (32, 64), nclip 0 and 3, on a
            noise image with a ramp, an offset and a few sources, for every histogram strategy of the node kernel
            (context option "noisemap_hist"), the strategies alternating in one process;
  torch     the same statistic as a torch composition on the device: the windows at the nodes with `unfold` (the
            interior nodes, whose windows are whole), torch.median - the lower median - twice, and for nclip 3 the
            clipped cells set to NaN and torch.nanmedian; scaled to the library's node count.  Not the same bits at the
            edges; a baseline for the time only;
  map       the map kernel - one node, so that the node kernel is a few microseconds - for out = image - background alone
            (16 B per cell) and for both maps and the S/N image (32 B per cell), against torch.sub over three N x N arrays
            (24 B per cell), 100 calls per timed window, the two in one process, torch.sub before and after.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/noisemap_timing.py [--reps 5] [--out profiles/noisemap_timing.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

N = 2400
CASES = [(16, 32), (32, 64)]
STRATEGIES = {0: "plain", 1: "prefix skip", 2: "copy per wave", 4: "wave aggregation", 5: "prefix skip + aggregation",
              6: "copy per wave + aggregation"}
STEPS = [("nodes", 500), ("torch", 300), ("map", 200)]


def timed(torch, work, reps, inner=1):
    """ms per call: `inner` calls between a pair of events, so that a short call's window is tens of milliseconds"""
    work()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            work()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms), "calls_per_window": inner}


def image(torch, dev):
    """noise whose sigma ramps from 1 to 4 across the field, offset 0.5, and 40 bright sources of 3 cells sigma"""
    g = torch.Generator(device=dev).manual_seed(3)
    img = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    img *= torch.linspace(1, 4, N, dtype=torch.float64, device=dev)
    img += 0.5
    pos = torch.randint(20, N - 20, (40, 2), device=dev, generator=g)
    ax = torch.arange(N, dtype=torch.float64, device=dev)
    for y, x in pos.tolist():
        img += 200.0 * torch.exp(-((ax[:, None] - y) ** 2 + (ax[None, :] - x) ** 2) / 18.0)
    return img


def torch_nodes(torch, img, step, half, kappa, nclip):
    side = 2 * half + 1
    first = step // 2 - half  # the first node whose window is whole
    i0 = max(0, -(first // step))
    lo = i0 * step + step // 2 - half
    w = img[lo:, lo:].unfold(0, side, step).unfold(1, side, step)
    nodes = w.shape[0] * w.shape[1]
    v = w.reshape(nodes, side * side).clone()
    for r in range(nclip + 1):
        med = torch.nanmedian(v, dim=1).values if r else torch.median(v, dim=1).values
        d = (v - med[:, None]).abs()
        mad = torch.nanmedian(d, dim=1).values if r else torch.median(d, dim=1).values
        if r < nclip:
            v[d > (kappa * (1.4826 * mad))[:, None]] = float("nan")
    return med, 1.4826 * mad, nodes


def step(what, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    img = image(torch, dev)
    base = {"N": N, "device": torch.cuda.get_device_name(0)}
    rows = []
    if what == "nodes":
        for st, half in CASES:
            G = len(gridhip.noise_grid(N, 0, st))
            for nclip in (0, 3):
                ms = {s: [] for s in STRATEGIES}
                stats = None
                for rep in range(reps + 1):  # (the first round is the warm-up; the strategies alternate)
                    for s in STRATEGIES:
                        ctx.set_option("noisemap_hist", s)
                        r = timed(torch, lambda: ctx.noise_map(img, step=st, half=half, nclip=nclip, maps=False), 1, inner=100)
                        if rep:
                            ms[s].append(r["median_ms"])
                ctx.set_option("noisemap_hist", 0)
                stats = ctx.noise_map(img, step=st, half=half, nclip=nclip, maps=False)[4].tolist()
                for s, label in STRATEGIES.items():
                    rows.append(dict(base, what="noise_map nodes", step=st, half=half, nclip=nclip, nodes=G * G, noisemap_hist=s,
                                     histogram=label, median_ms=statistics.median(ms[s]), min_ms=min(ms[s]), max_ms=max(ms[s]),
                                     reps=len(ms[s]), calls_per_window=100, stats=stats))
    elif what == "torch":
        for st, half in CASES:
            G = len(gridhip.noise_grid(N, 0, st))
            for nclip in (0, 3):
                nodes = torch_nodes(torch, img, st, half, 3.0, nclip)[2]
                r = timed(torch, lambda: torch_nodes(torch, img, st, half, 3.0, nclip), reps, inner=2)
                rows.append(dict(base, what="torch unfold + median", step=st, half=half, nclip=nclip, nodes=nodes, **r,
                                 scratch_mb=nodes * (2 * half + 1) ** 2 * 8 / 1e6, library_nodes=G * G,
                                 scaled_ms=r["median_ms"] * G * G / nodes))
    else:
        bg, out = torch.zeros_like(img), torch.empty_like(img)
        one = dict(step=N, half=1, min_count=1, nclip=0)  # one node of 9 cells
        sub = lambda: torch.sub(img, bg, out=out)  # noqa: E731
        rows.append(dict(base, what="torch.sub", case="before", bytes_per_cell=24, **timed(torch, sub, reps, inner=100)))
        for name, kw, nbytes in (("image - background", dict(mode="subtract", maps=False, out=out), 16),
                                 ("both maps and S/N", dict(mode="snr", maps=True, out=out), 32)):
            r = timed(torch, lambda: ctx.noise_map(img, **one, **kw), reps, inner=100)
            rows.append(dict(base, what="noise_map maps", case=name, bytes_per_cell=nbytes, launches=3, **r,
                             gb_per_s=N * N * nbytes / (r["median_ms"] * 1e-3) / 1e9))
        rows.append(dict(base, what="torch.sub", case="after", bytes_per_cell=24, **timed(torch, sub, reps, inner=100)))
        for r in (rows[0], rows[-1]):
            r["gb_per_s"] = N * N * 24 / (r["median_ms"] * 1e-3) / 1e9
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisemap_timing.jsonl"))
    ap.add_argument("--step", help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(args.step, args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for what, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
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
    return 0 if len(rows) and {r["what"] for r in rows} >= {"noise_map nodes", "torch unfold + median", "noise_map maps"} else 1


if __name__ == "__main__":
    sys.exit(main())
