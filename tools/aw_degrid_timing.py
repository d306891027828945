#!/usr/bin/env python3
"""aw degrid and aw plans on cfg4's stream (10^6 visibilities, 4096^2, 15 x 15, Q = 8, 128 planes, 512 antennas; the
stream, kernels and antenna kernels of bench.py): device time per call of awgrid_dev and awdegrid_dev, of plan
creation, and per pass of plan grid / plan degrid, with the tap-reusing (sort = 0) and the general (sort = 2) tile
kernel for the degrid pass.  Device events on torch's stream, warm-up calls first, the median of --reps timed ones.
usage: python tools/aw_degrid_timing.py [--reps 20] [--warmup 3] [--out profiles/aw_degrid_cfg4.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
import torch  # noqa: E402

import bench  # noqa: E402
import gridhip  # noqa: E402


def timed(fn, reps, warmup):
    """device milliseconds of fn() per call: warm-up calls, then `reps` calls each between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aw_degrid_cfg4.jsonl"))
    args = ap.parse_args()
    n, N, W, Q, S = bench.WORKLOADS["cfg4"]
    A = bench.AW_ANTENNAS
    dev = torch.device("cuda:0")
    wk = bench.synth_kernels(W, Q, S, dev)
    ak = bench.synth_akernels(A, S, dev)
    u, v, wb, a1, a2, vis = bench.synth_aw_stream(n, N, W, S, A, 0x5EEDC0DE, dev)
    p, idx = (u, v, None), (wb, a1, a2)
    ctx = gridhip.Context(0)
    grid = torch.zeros((N, N), dtype=torch.complex128, device=dev)
    model = torch.complex(torch.randn(N, N, device=dev, dtype=torch.float64),
                          torch.randn(N, N, device=dev, dtype=torch.float64))
    out = torch.empty(n, dtype=torch.complex128, device=dev)
    head = {"workload": "cfg4", "n": n, "N": N, "W": W, "Q": Q, "S": S, "A": A, "device": torch.cuda.get_device_name(0)}
    rows = []

    def rec(what, r, **extra):
        row = dict(head, what=what, **r, **extra)
        rows.append(row)
        print(json.dumps(row), flush=True)

    rec("awgrid_dev per call", timed(lambda: ctx.convgrid4(wk, ak, grid, p, idx, vis), args.reps, args.warmup))
    st = ctx.aw_stats(S)
    for sort, name in ((0, "sorted"), (2, "general")):
        ctx.set_option("sort", sort)
        rec(f"awdegrid_dev per call ({name})", timed(lambda: ctx.degrid4(wk, ak, model, p, idx, out=out), args.reps,
                                                     args.warmup), last_path=ctx.get_option("last_path"))
    ctx.set_option("sort", 0)
    ref = ctx.degrid4(wk, ak, model, p, idx)
    # plan creation (synchronises: wall clock as well as events)
    cre, wall = [], []
    for i in range(args.warmup + max(3, args.reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pl = ctx.aw_plan((N, N), wk, ak, p, idx)
        b.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            cre.append(a.elapsed_time(b))
            wall.append((time.perf_counter() - t0) * 1e3)
        pl.close()
    rec("aw plan create", {"median_ms": statistics.median(cre), "min_ms": min(cre), "max_ms": max(cre),
                           "reps": len(cre), "wall_median_ms": statistics.median(wall)})
    for sort, name in ((0, "sorted"), (2, "general")):
        ctx.set_option("sort", sort)
        pl = ctx.aw_plan((N, N), wk, ak, p, idx)
        rec(f"aw plan grid per pass ({name})", timed(lambda: pl.grid(grid, vis), args.reps, args.warmup))
        path = ctx.get_option("last_path")
        r = timed(lambda: pl.degrid(model, out=out), args.reps, args.warmup)
        torch.cuda.synchronize()
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        rec(f"aw plan degrid per pass ({name})", r, last_path=ctx.get_option("last_path"), grid_last_path=path,
            rel_err_vs_awdegrid=err)
        pl.close()
    ctx.set_option("sort", 0)
    rows.append(dict(head, what="aw stats of awgrid_dev", **{k: st[k] for k in ("vis_keyed", "kernels_built", "hit_rate")}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
