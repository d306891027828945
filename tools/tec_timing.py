#!/usr/bin/env python3
"""Dispersive delay (TEC) calibration against torch, device events after a warm-up, the median of `reps` runs, at 2016
baselines (64 antennas), T = 64, tint = 8 (8 intervals), F = 256 channels over 120-180 MHz, Nd = 1024 delays, Nm = 64 TEC
cells (a cube of 0.53 GB); a point source seen through per-antenna clock delays, TEC and phases, and noise:
  search    ctx.tec_search over the whole grid and over the 5 x 5 cells around the grid's zero;
  matmul    a torch composition of the same product: Xbar = the sum over an interval, then per interval the batched complex
            matmul Ef^T (diag(Xbar) Em), abs, argmax (rocBLAS; a scratch cube of [B, Nd, Nm] per interval).  Not the same
            bits; a baseline for the time only;
  fit       ctx.tecfit with three rounds (window 2 x 2);
  apply     ctx.apply_tec against torch.mul over the same bytes, 100 calls per timed window (40 for the 5 x 5 search), the
            two in one process, apply_tec before and after.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/tec_timing.py [--reps 5] [--out profiles/tec_timing.jsonl]"""
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

A, T, TINT, F, PAD, NM = 64, 64, 8, 256, 4, 64
STEPS = [("search", 300), ("matmul", 300), ("fit", 300), ("apply", 200)]


def sky(torch, gridhip, dev):
    """freq, a1, a2, vis [B][T][F]: a unit point source through random antenna terms, constant over an interval, and noise"""
    g = torch.Generator(device=dev).manual_seed(7)
    freq = torch.linspace(120.0e6, 180.0e6, F, dtype=torch.float64, device=dev)
    iu = torch.triu_indices(A, A, 1, device=dev)
    a1, a2 = iu[0].contiguous(), iu[1].contiguous()
    I = T // TINT
    df = 60.0e6 / (F - 1)
    clock = (torch.rand((I, A), dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.1 / df
    tec = (torch.rand((I, A), dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.4
    ph = 2 * math.pi * torch.rand((I, A), dtype=torch.float64, device=dev, generator=g)
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    z = -gridhip.TEC_KAPPA * (1.0 / freq - 1.0 / nu0)
    psi = ph[:, :, None] + 2 * math.pi * (clock[:, :, None] * (freq - nu0)[None, None, :] + tec[:, :, None] * z[None, None, :])
    dpsi = (psi[:, a1] - psi[:, a2]).permute(1, 0, 2)  # [B][I][F]
    dpsi = dpsi[:, :, None, :].expand(-1, -1, TINT, -1).reshape(a1.numel(), T, F)
    vis = torch.polar(torch.ones((a1.numel(), T, F), dtype=torch.float64, device=dev), dpsi.contiguous())
    vis += 0.5 * torch.complex(torch.randn(vis.shape, dtype=torch.float64, device=dev, generator=g),
                               torch.randn(vis.shape, dtype=torch.float64, device=dev, generator=g))
    return freq, a1, a2, vis.contiguous()


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
    freq, a1, a2, vis = sky(torch, gridhip, dev)
    B, I = int(a1.numel()), T // TINT
    delays, tecs = gridhip.tec_grid(freq.cpu().numpy(), 0.5, pad=PAD)
    tecs = (-(NM // 2) * tecs[1], tecs[1], NM)
    Nd, Nm = delays[2], tecs[2]
    base = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "tint": TINT, "F": F, "Nd": Nd, "Nm": Nm,
            "cube_GB": round(B * T * F * 16 / 1e9, 2)}
    ctx = gridhip.Context(0)
    tab = ctx.tec_tables(freq, T, TINT, delays, tecs)
    rows = []
    if what == "search":
        peaks = torch.empty((B, I, 12), dtype=torch.float64, device=dev)
        for name, cells in (("whole grid", None), ("5 x 5 cells", (Nd // 2 - 2, Nd // 2 + 3, Nm // 2 - 2, Nm // 2 + 3))):
            res = ctx.tec_search(vis, tab, a1, a2, A, TINT, delays, tecs, cells=cells, peaks=peaks)
            r = timed(torch, lambda: ctx.tec_search(vis, tab, a1, a2, A, TINT, delays, tecs, cells=cells, peaks=peaks), reps,
                      inner=1 if cells is None else 40)
            nj, nm = (Nd, Nm) if cells is None else (5, 5)
            mac = 8.0 * B * I * F * nj * nm            # the ordered sum: 8 fp64 instructions per complex multiply-add
            prod = 6.0 * B * I * F * nm * (nj / 2.0)   # the Em Xbar products: one per (f, m) and pair of delays
            rows.append(dict(base, what="tec_search_dev", case=name, tile=list(gridhip.tec_tile()), stats=res[1].tolist(),
                             mean_coh2=float(res[0][:, :, 7].mean()), fp64_instr_per_s=(mac + prod) / (r["median_ms"] * 1e-3),
                             mac_instr_per_s=mac / (r["median_ms"] * 1e-3), **r))
    elif what == "matmul":
        n = 2 * F * Nd
        Ef = torch.view_as_complex(tab[16:16 + n].reshape(F, Nd, 2))
        Em = torch.view_as_complex(tab[16 + n:16 + n + 2 * F * Nm].reshape(F, Nm, 2))
        EfT = Ef.t().contiguous()

        def work():
            xbar = vis.reshape(B, I, TINT, F).sum(dim=2)
            best = []
            for i in range(I):  # an interval at a time: the scratch cube is [B, Nd, Nm]
                S = torch.matmul(EfT, xbar[:, i, :, None] * Em)
                best.append(S.abs().reshape(B, -1).argmax(dim=1))
            return best
        rows.append(dict(base, what="torch", case="sum over the interval, batched complex matmul Ef^T (diag(Xbar) Em), abs, argmax",
                         scratch_GB=round(B * Nd * Nm * 24 / 1e9, 2), **timed(torch, work, reps)))
    elif what == "fit":
        res = ctx.tecfit(vis, tab, a1, a2, A, TINT, delays, tecs, rounds=3, window=(2, 2), niter=50)
        r = timed(torch, lambda: ctx.tecfit(vis, tab, a1, a2, A, TINT, delays, tecs, rounds=3, window=(2, 2), niter=50), reps)
        rows.append(dict(base, what="tecfit_dev", case="three rounds, window 2 x 2, niter 50", stats=res[3].tolist(), **r))
    else:
        sol = ctx.tecfit(vis, tab, a1, a2, A, TINT, delays, tecs, rounds=3)[0]
        wt = torch.ones((B, T, F), dtype=torch.float64, device=dev)
        out, wout = torch.empty_like(vis), torch.empty_like(wt)
        apply = lambda: ctx.apply_tec(sol, tab, vis, a1, a2, TINT, weights=wt, out=out, weights_out=wout)  # noqa: E731
        r = timed(torch, apply, reps, inner=100)
        rows.append(dict(base, what="apply_tec_dev", case="vis and weights", avg_after=float(out.mean(dim=(1, 2)).abs().mean()),
                         avg_before=float(vis.mean(dim=(1, 2)).abs().mean()), **r))
        other = torch.polar(torch.ones((B, T, F), dtype=torch.float64, device=dev), torch.zeros((B, T, F), dtype=torch.float64, device=dev))

        def mul():
            torch.mul(vis, other, out=out)
            wout.copy_(wt)
        rows.append(dict(base, what="torch", case="torch.mul by a given cube of phasors, and the copy of the weights",
                         **timed(torch, mul, reps, inner=100)))
        # the two once more in the other order, in the same process: windows of 100 calls each
        rows.append(dict(base, what="apply_tec_dev", case="vis and weights, after torch.mul", **timed(torch, apply, reps, inner=100)))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tec_timing.jsonl"))
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
