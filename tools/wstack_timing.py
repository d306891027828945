#!/usr/bin/env python3
"""W-stacking against w-projection on one stream, on the GPU and under no profiler.
  The stream: n visibilities, u, v uniform in +-0.4 lam, w uniform in +-wmax, theta = 0.1, so that the w-kernel of the full
  range spreads over about wmax theta^2 = 20 cells more than the one of w = 0.
  kind 2   do_imaging with ("w_cache", S = 31): one kernel per w-plane of the whole stream at the support the full w range
           needs (15 + wmax theta^2 cells, the next odd size the tap-reusing kernel takes), and at S = 15 for comparison
           (the support w-stacking runs at; at this w range it truncates the kernels).  The code of kind 2 is the parent
           commit's, unchanged.
  stacked  do_imaging with ("wstack", S = 15, planes = M) for M = 4, 8, 16: the kernels carry M wstep / 2 of |w| only.
           Beside the whole call: the creation of a stack (partition, one binning per layer, the kernel table), one image
           pass and one predict pass of a bound stack.
  per layer  a stack of L layers with ONE visibility each: its image pass is L times (a tile pass over nothing, the
           transform, the screen kernel - which also clears the grid, so there is no clear pass to time).  The events give
           the sum per layer; its split into transform and screen is read from the kernel statistics of this very step
           under a profiler (rocprofv3 --kernel-trace --stats -- python tools/wstack_timing.py --step layers,32).  The
           screen's traffic floor is 40 B per cell (16 read, 16 written as zeros, 8 of the image) at 6.29 TB/s.
Events on the stream around eager calls, a warm-up first, the median and the extremes of `reps` runs.  Every step is a
process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of time ends the run.
usage: python tools/wstack_timing.py [--reps 5] [--nvis 4000000] [--out profiles/wstack_timing.jsonl]  (--out is appended to)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE = 6.29e12
THETA, LAM, NVIS, WSTEP, WMAX, QPX, NPIXFF = 0.1, 20480, 4_000_000, 100, 2000.0, 4, 64
STEPS = ["w_cache,31", "w_cache,15", "wstack,4", "wstack,8", "wstack,16", "layers,32"]


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def stream(torch, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    r = lambda lo, hi: torch.rand(NVIS, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo  # noqa: E731
    u, v, w = r(-0.4 * LAM, 0.4 * LAM), r(-0.4 * LAM, 0.4 * LAM), r(-WMAX, WMAX)
    vis = torch.complex(torch.randn(NVIS, dtype=torch.float64, device=dev, generator=gen),
                        torch.randn(NVIS, dtype=torch.float64, device=dev, generator=gen))
    return (u, v, w), vis


def step(what, arg, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    N = ctx.image_size(THETA, LAM)
    row = {"step": what, "N": N, "n": NVIS, "theta": THETA, "wstep": WSTEP, "wmax": WMAX, "qpx": QPX, "npixFF": NPIXFF,
           "device": torch.cuda.get_device_name(0)}
    if what == "w_cache":
        uvw, vis = stream(torch, dev)
        ko = dict(wstep=WSTEP, qpx=QPX, npixFF=NPIXFF, npixKern=arg)
        row.update(S=arg, do_imaging=timed(torch, lambda: ctx.do_imaging(THETA, LAM, uvw, None, None, None, None, vis,
                                                                        ("w_cache", ko)), reps))
        row["last_path"] = ctx.get_option("last_path")
    elif what == "wstack":
        uvw, vis = stream(torch, dev)
        ko = dict(wstep=WSTEP, planes=arg, qpx=QPX, npixFF=NPIXFF, npixKern=15)
        row.update(S=15, planes=arg)
        row["do_imaging"] = timed(torch, lambda: ctx.do_imaging(THETA, LAM, uvw, None, None, None, None, vis, ("wstack", ko)),
                                  reps)
        row["create"] = timed(torch, lambda: ctx.wstack(THETA, LAM, uvw, ko).close(), max(3, reps // 2))
        ws = ctx.wstack(THETA, LAM, uvw, ko)
        img = torch.empty((N, N), dtype=torch.float64, device=dev)
        out = torch.empty(NVIS, dtype=torch.complex128, device=dev)
        model = torch.randn((N, N), dtype=torch.float64, device=dev)
        row.update(layers=ws.layers, occupied=ws.occupied, dropped=ws.dropped)
        row["image_pass"] = timed(torch, lambda: ws.image(vis, out=img), reps)
        row["last_path"] = ctx.get_option("last_path")
        row["predict_pass"] = timed(torch, lambda: ws.predict(model, out=out), reps)
        ws.close()
    else:  # layers: one visibility per layer
        L = arg
        w = (torch.arange(L, dtype=torch.float64, device=dev) - L // 2) * WSTEP
        z = torch.zeros(L, dtype=torch.float64, device=dev)
        ko = dict(wstep=WSTEP, planes=1, qpx=QPX, npixFF=NPIXFF, npixKern=15)
        ws = ctx.wstack(THETA, LAM, (z, z, w), ko)
        assert (ws.layers, ws.occupied) == (L, L)
        vis = torch.ones(L, dtype=torch.complex128, device=dev)
        img = torch.empty((N, N), dtype=torch.float64, device=dev)
        t = timed(torch, lambda: ws.image(vis, out=img), reps)
        floor_ms = N * N * 40 / COPY_RATE * 1e3
        row.update(layers=L, image_pass=t, per_layer_ms=t["median_ms"] / L, screen_floor_ms=floor_ms, clear_ms=0.0,
                   note="the screen kernel clears the grid: there is no clear pass")
        ws.close()
    ctx.close()
    return row


def main():
    global NVIS
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wstack_timing.jsonl"))
    ap.add_argument("--nvis", type=int, default=NVIS)
    ap.add_argument("--step", metavar="what,arg", help="run one step in this process (internal)")
    args = ap.parse_args()
    NVIS = args.nvis
    if args.step:
        what, arg = args.step.split(",")
        print("ROW " + json.dumps(step(what, int(arg), args.reps)), flush=True)
        return 0
    rows = []
    for s in STEPS:
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--nvis", str(NVIS), "--step", s], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {s} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
