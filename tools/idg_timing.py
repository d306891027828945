#!/usr/bin/env python3
"""Image-domain layers against w-projection layers of the same stack: time and accuracy in one table, on the GPU and under
no profiler.
  The stream: n visibilities, u, v uniform in +-0.4 lam, w uniform in +-2000, theta = 0.1, lam = 20480 (N = 2048),
  wstep = 100, 8 planes per layer.  The visibilities are the exact ones (Context.dft_predict) of a few points off their
  cells' centres in the inner half of the field.
  Configurations: ("idg", subgrid, margin) for (16, 8), (24, 12), (32, 16) and ("wstack", qpx 4, npixFF 64) at support 15
  and 31, all on the same stream in the same process.
  Per configuration: creation (one call, host clock, synchronised), WStack.image, WStack.predict and Imager.cycle(vis, model)
  timed in turns over the configurations - so that a drift falls on all of them alike - with events on the stream, one
  warm-up each, the median and the extremes of `reps` runs.
  Accuracy: err = max |image - direct| / max |direct| over probe cells (the points' own cells and random cells of the inner
  half), `direct` the direct Fourier sum N^-2 sum_k vis_k exp(2 pi i (u_k l + v_k m - w_k (1 - sqrt(1 - l^2 - m^2)))) at
  those cells, computed with torch on the device; `image` is WStack.image (natural weights, no normalisation).
Every n is a process of its own under `timeout`, and the steps are chained: one that fails, faults or runs out of time ends
the run.
usage: python tools/idg_timing.py [--reps 5] [--sizes 4000000,32000000] [--out profiles/idg_timing.jsonl]  (--out is appended to)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

THETA, LAM, WSTEP, WMAX, M = 0.1, 20480, 100, 2000.0, 8
SIZES = [4_000_000, 32_000_000]
CONFIGS = {
    "idg_16_8": ("idg", dict(wstep=WSTEP, planes=M, subgrid=16, margin=8)),
    "idg_24_12": ("idg", dict(wstep=WSTEP, planes=M, subgrid=24, margin=12)),
    "idg_32_16": ("idg", dict(wstep=WSTEP, planes=M, subgrid=32, margin=16)),
    "wstack_S15": ("wstack", dict(wstep=WSTEP, planes=M, qpx=4, npixFF=64, npixKern=15)),
    "wstack_S31": ("wstack", dict(wstep=WSTEP, planes=M, qpx=4, npixFF=64, npixKern=31)),
}
NPROBE = 192


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed_in_turns(torch, fns, reps):
    """{name: summary} of the callables, run in turns after one warm-up each"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: summary(v) for k, v in ms.items()}


def direct_sum(torch, u, v, w, vis, N, cells):
    """the direct Fourier sum at the (y, x) probe cells, in chunks of the stream"""
    c = (cells.to(torch.float64) - N // 2) / N * THETA
    cy, cx = c[:, 0:1], c[:, 1:2]
    ph = 1.0 - torch.sqrt(1.0 - cx * cx - cy * cy)
    out = torch.zeros(len(cells), dtype=torch.complex128, device=u.device)
    step = 1 << 18
    for k in range(0, len(u), step):
        s = slice(k, k + step)
        p = cx * u[s] + cy * v[s] - ph * w[s]
        p = 2.0 * torch.pi * (p - torch.round(p))
        out += (torch.complex(torch.cos(p), torch.sin(p)) * vis[s]).sum(dim=1)
    return out / (N * N)


def step(n, reps):
    import numpy as np
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    N = ctx.image_size(THETA, LAM)
    gen = torch.Generator(device=dev).manual_seed(5)
    r = lambda lo, hi: torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo  # noqa: E731
    u, v, w = r(-0.4 * LAM, 0.4 * LAM), r(-0.4 * LAM, 0.4 * LAM), r(-WMAX, WMAX)
    rng = np.random.default_rng(9)
    npts = 5
    pts = rng.uniform(N // 4 + 8, N - N // 4 - 8, (npts, 2))  # (y, x), off the cells' centres, in the inner half
    flux = rng.uniform(0.5, 1.5, npts)
    pos = (pts - N // 2) / N * THETA
    comps = torch.from_numpy(gridhip.components(pos[:, 1], pos[:, 0], flux)).to(dev)
    vis = ctx.dft_predict((u, v, w), comps).clone()
    model = torch.zeros((N, N), dtype=torch.float64, device=dev)
    for (y, x), f in zip(np.rint(pts).astype(int), flux):
        model[y, x] = f
    cells = np.concatenate([np.rint(pts).astype(np.int64), rng.integers(N // 4, N - N // 4, (NPROBE - npts, 2))])
    cells_d = torch.from_numpy(cells).to(dev)
    direct = direct_sum(torch, u, v, w, vis, N, cells_d)
    row = {"N": N, "n": n, "theta": THETA, "wstep": WSTEP, "wmax": WMAX, "planes": M, "points": npts, "probe_cells": NPROBE,
           "device": torch.cuda.get_device_name(0), "idg_chunk": ctx.get_option("idg_chunk"),
           "idg_split": ctx.get_option("idg_split"), "configs": {}}
    img = torch.empty((N, N), dtype=torch.float64, device=dev)
    pred, res = torch.empty_like(vis), torch.empty_like(vis)
    stacks, imagers = {}, {}
    for name, f in CONFIGS.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stacks[name] = ctx.wstack(THETA, LAM, (u, v, w), f)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        imagers[name] = ctx.imager(THETA, LAM, (u, v, w), f)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ws = stacks[name]
        got = ws.image(vis, out=img)[cells_d[:, 0], cells_d[:, 1]]
        err = float((got - direct.real).abs().max() / direct.real.abs().max())
        row["configs"][name] = {"imgfn": [f[0], f[1]], "layers": ws.layers, "occupied": ws.occupied, "dropped": ws.dropped,
                                "create_stack_ms": (t1 - t0) * 1e3, "create_imager_ms": (t2 - t1) * 1e3, "image_error": err}
    for what, fns in (("image", {k: (lambda s=s: s.image(vis, out=img)) for k, s in stacks.items()}),
                      ("predict", {k: (lambda s=s: s.predict(model, out=pred)) for k, s in stacks.items()}),
                      ("cycle", {k: (lambda i=i: i.cycle(vis, model, out=img, vis_res=res)) for k, i in imagers.items()})):
        for k, t in timed_in_turns(torch, fns, reps).items():
            row["configs"][k][what] = t
    for x in list(stacks.values()) + list(imagers.values()):
        x.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idg_timing.jsonl"))
    ap.add_argument("--step", metavar="n", help="run one size in this process (internal)")
    args = ap.parse_args()
    if args.step:
        print("ROW " + json.dumps(step(int(args.step), args.reps)), flush=True)
        return 0
    rows = []
    for n in [int(x) for x in args.sizes.split(",")]:
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--step", str(n)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {n} ended with status {r.returncode}: nothing more is started", flush=True)
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
