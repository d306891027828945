#!/usr/bin/env python3
"""Delay and rate calibration against torch, device events after a warm-up, the median of `reps` runs, at 2016 baselines (64
antennas), T = 64, F = 256, Nd = 1024 delays, Nr = 256 rates, one solution interval (a cube of 0.53 GB); a point source seen
through per-antenna delays, rates and phases, and noise:
  search    ctx.fringe_search over the whole grid and over the 8 x 8 cells around the grid's zero;
  fft       a torch composition of the same search: fft2 of the cube zero-padded to [Nr, Nd] (an 8.5 GB cube), abs, argmax.
            Uniform channels only, not the same bits; a baseline for the time only;
  fit       ctx.fringefit with three rounds (window 2 x 2);
  apply     ctx.apply_fringe against torch.mul over the same bytes, 100 calls per timed window (40 for the 8 x 8 search), the
            two in one process, apply_fringe before and after.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/fringe_timing.py [--reps 5] [--out profiles/fringe_timing.jsonl]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

A, T, F, PAD = 64, 64, 256, 4
STEPS = [("search", 300), ("fft", 300), ("fit", 300), ("apply", 200)]


def sky(torch, dev):
    """freq, time, a1, a2, vis [B][T][F]: a unit point source through random antenna terms, and noise"""
    g = torch.Generator(device=dev).manual_seed(7)
    freq = 1.0e9 + 1.0e6 * torch.arange(F, dtype=torch.float64, device=dev)
    time = 2.0 * torch.arange(T, dtype=torch.float64, device=dev)
    iu = torch.triu_indices(A, A, 1, device=dev)
    a1, a2 = iu[0].contiguous(), iu[1].contiguous()
    tau = (torch.rand(A, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.1 / 1.0e6
    rate = (torch.rand(A, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.1 / 2.0
    ph = 2 * math.pi * torch.rand(A, dtype=torch.float64, device=dev, generator=g)
    nu0, tref = freq[0] + 0.5 * (freq[-1] - freq[0]), time[0] + 0.5 * (time[-1] - time[0])
    psi = ph[:, None, None] + 2 * math.pi * (tau[:, None, None] * (freq - nu0)[None, None, :]
                                             + rate[:, None, None] * (time - tref)[None, :, None])
    vis = torch.polar(torch.ones((a1.numel(), T, F), dtype=torch.float64, device=dev), psi[a1] - psi[a2])
    vis += 0.5 * torch.complex(torch.randn(vis.shape, dtype=torch.float64, device=dev, generator=g),
                               torch.randn(vis.shape, dtype=torch.float64, device=dev, generator=g))
    return freq, time, a1, a2, vis.contiguous()


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


def step(what, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    freq, time, a1, a2, vis = sky(torch, dev)
    B = int(a1.numel())
    delays, rates = gridhip.fringe_grid(freq.cpu().numpy(), time.cpu().numpy(), 0, pad=PAD)
    Nd, Nr = delays[2], rates[2]
    base = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "F": F, "Nd": Nd, "Nr": Nr, "cube_GB": round(B * T * F * 16 / 1e9, 2)}
    ctx = gridhip.Context(0)
    tab = ctx.fringe_tables(freq, time, 0, delays, rates)
    rows = []
    if what == "search":
        peaks = torch.empty((B, 1, 12), dtype=torch.float64, device=dev)
        for name, cells in (("whole grid", None), ("8 x 8 cells", (Nd // 2 - 4, Nd // 2 + 4, Nr // 2 - 4, Nr // 2 + 4))):
            res = ctx.fringe_search(vis, tab, a1, a2, A, 0, delays, rates, cells=cells, peaks=peaks)
            r = timed(torch, lambda: ctx.fringe_search(vis, tab, a1, a2, A, 0, delays, rates, cells=cells, peaks=peaks), reps,
                      inner=1 if cells is None else 40)
            nj, nk = (Nd, Nr) if cells is None else (8, 8)
            instr = 8.0 * B * T * nj * (F + nk)  # the two sums, 8 fp64 instructions per complex multiply-add
            rows.append(dict(base, what="fringe_search_dev", case=name, tile=list(gridhip.fringe_tile()), stats=res[1].tolist(),
                             mean_coh2=float(res[0][:, 0, 7].mean()), fp64_instr_per_s=instr / (r["median_ms"] * 1e-3), **r))
    elif what == "fft":
        def work():
            S = torch.fft.fft2(vis, s=(Nr, Nd))
            return S.abs().reshape(B, -1).argmax(dim=1)
        rows.append(dict(base, what="torch", case="fft2 zero-padded to [Nr, Nd], abs, argmax",
                         scratch_GB=round(B * Nr * Nd * 16 / 1e9, 2), **timed(torch, work, reps)))
    elif what == "fit":
        res = ctx.fringefit(vis, tab, a1, a2, A, 0, delays, rates, rounds=3, window=(2, 2), niter=50)
        r = timed(torch, lambda: ctx.fringefit(vis, tab, a1, a2, A, 0, delays, rates, rounds=3, window=(2, 2), niter=50), reps)
        rows.append(dict(base, what="fringefit_dev", case="three rounds, window 2 x 2, niter 50", stats=res[3].tolist(), **r))
    else:
        sol = ctx.fringefit(vis, tab, a1, a2, A, 0, delays, rates, rounds=2)[0]
        wt = torch.ones((B, T, F), dtype=torch.float64, device=dev)
        out, wout = torch.empty_like(vis), torch.empty_like(wt)
        apply = lambda: ctx.apply_fringe(sol, tab, vis, a1, a2, 0, weights=wt, out=out, weights_out=wout)  # noqa: E731
        r = timed(torch, apply, reps, inner=100)
        rows.append(dict(base, what="apply_fringe_dev", case="vis and weights", avg_after=float(out.mean(dim=(1, 2)).abs().mean()),
                         avg_before=float(vis.mean(dim=(1, 2)).abs().mean()), **r))
        other = torch.polar(torch.ones((B, T, F), dtype=torch.float64, device=dev), torch.zeros((B, T, F), dtype=torch.float64, device=dev))

        def mul():
            torch.mul(vis, other, out=out)
            wout.copy_(wt)
        rows.append(dict(base, what="torch", case="torch.mul by a given cube of phasors, and the copy of the weights",
                         **timed(torch, mul, reps, inner=100)))
        # the two once more in the other order, in the same process: windows of 100 calls each
        rows.append(dict(base, what="apply_fringe_dev", case="vis and weights, after torch.mul", **timed(torch, apply, reps, inner=100)))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fringe_timing.jsonl"))
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
    return 0 if len(rows) >= 7 else 1


if __name__ == "__main__":
    sys.exit(main())
