#!/usr/bin/env python3
"""One iteration of the direction-dependent solver at n = 5.76 x 10^6 visibilities (the size tools/flag_timing.py uses),
T = 16 solution intervals, time-major, for A = 64 and A = 512 antennas and D = 1, 2, 4, 8 directions:
  ddcal    ctx.ddcal on device tensors with tol = 0 at niter = K and niter = 2 K: the difference of the two medians over K
           is one iteration (the streaming kernel plus the one-work-group solve) without the prepare pass, the rotation
           and the chi^2 pass.  Events around eager calls, warm-up first, the median and the extremes of `reps` runs.
  gaincal  ctx.gaincal measured the same way in the same process on the direction-0 model: the yardstick beside D = 1.
Next to each figure the bytes an iteration streams - 32 + 16 D per visibility (key 8, s V 16, s 8, D model values; gaincal:
32) - the time those bytes take at 6.29 TB/s (the measured copy rate; the HBM peak is 8 TB/s), and the ratio of the two.
At this n the streams are 0.28 GB (D = 1) to 0.92 GB (D = 8): D = 1 sits at the edge of the 256 MiB Infinity Cache, so
its rate is not an HBM rate.  Which path ran (LDS, or - A above gridhip.ddcal_lds_antennas(D), here A = 512 at D = 8 - the
global table) and the work-group size are recorded.
Every A is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of time
ends the run, and nothing more is started on the device.
usage: python tools/ddcal_timing.py [--reps 7] [--out profiles/ddcal_n5760000.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE, HBM_PEAK = 6.29e12, 8.0e12
N, T, K = 5_760_000, 16, 4
ANTENNAS, DIRECTIONS = [64, 512], [1, 2, 4, 8]


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


def iteration(torch, solve, reps, bytes_per_vis, n):
    t1, t2 = timed(torch, lambda: solve(K), reps), timed(torch, lambda: solve(2 * K), reps)
    it_ms = (t2["median_ms"] - t1["median_ms"]) / K
    spread = ((t2["max_ms"] - t1["min_ms"]) / K, (t2["min_ms"] - t1["max_ms"]) / K)
    floor_ms = bytes_per_vis * n / COPY_RATE * 1e3
    return {"solve_K": t1, "solve_2K": t2, "K": K, "iteration_ms": it_ms, "iteration_ms_spread": [min(spread), max(spread)],
            "bytes_per_vis": bytes_per_vis, "ms_at_copy_rate": floor_ms, "iteration_over_copy_rate": it_ms / floor_ms,
            "effective_GBps": bytes_per_vis * n / (it_ms * 1e-3) / 1e9}


def step(A, reps, n):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(A)
    ctx = gridhip.Context(0)
    Dmax = max(DIRECTIONS)
    a1 = torch.randint(0, A, (n,), device=dev, generator=gen)
    a2 = (a1 + torch.randint(1, A, (n,), device=dev, generator=gen)) % A
    slot = (torch.arange(n, device=dev) * T) // n  # time-major: T equal runs
    u, v = (600 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 300 for _ in range(2))
    l, m = (0.1 * torch.rand(Dmax, 1, dtype=torch.float64, device=dev, generator=gen) - 0.05 for _ in range(2))
    M = torch.exp(-2j * torch.pi * (u * l + v * m)) * (1 + 2 * torch.rand(Dmax, 1, dtype=torch.float64, device=dev, generator=gen))
    gt = (1 + 0.2 * torch.randn(Dmax, T, A, dtype=torch.float64, device=dev, generator=gen)) * torch.exp(
        1j * (2 * torch.rand(Dmax, T, A, dtype=torch.float64, device=dev, generator=gen) - 1))
    rows = []
    g1 = torch.ones(T, A, dtype=torch.complex128, device=dev)
    V1 = gt[0][slot, a1] * M[0] * gt[0][slot, a2].conj()

    def gaincal(niter):
        g1.fill_(1.0)
        return ctx.gaincal(V1, M[0], a1, a2, A, slot=slot, nslots=T, niter=niter, tol=0.0, gains=g1)
    base = iteration(torch, gaincal, reps, 32, n)
    rows.append({"solver": "gaincal", "n": n, "A": A, "T": T, "D": 1, "device": torch.cuda.get_device_name(0), **base})
    for D in DIRECTIONS:
        Md = M[:D].contiguous()
        V = sum(gt[d][slot, a1] * Md[d] * gt[d][slot, a2].conj() for d in range(D))
        V = V + 0.1 * torch.randn(n, dtype=torch.complex128, device=dev, generator=gen)
        g = torch.ones(D, T, A, dtype=torch.complex128, device=dev)

        def ddcal(niter):
            g.fill_(1.0)
            return ctx.ddcal(V, Md, a1, a2, A, slot=slot, nslots=T, niter=niter, tol=0.0, gains=g)
        row = iteration(torch, ddcal, reps, 32 + 16 * D, n)
        lds = A <= gridhip.ddcal_lds_antennas(D)
        table = A * (D * D + 4 * D) * 8
        rows.append({"solver": "ddcal", "n": n, "A": A, "T": T, "D": D, "device": torch.cuda.get_device_name(0),
                     "path": "lds" if lds else "global", "lds_bytes": table if lds else 0,
                     "work_group": (256 if 4 * (table + 64) <= 160 * 1024 else 512 if 2 * (table + 64) <= 160 * 1024 else 1024)
                     if lds else 256, "iteration_over_gaincal": row["iteration_ms"] / base["iteration_ms"],
                     "stats": ddcal(2 * K)[1].cpu().tolist(), **row})
        del V, g, Md
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddcal_n5760000.jsonl"))
    ap.add_argument("--step", metavar="A", help="run one antenna count in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(int(args.step), args.reps, args.n):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for A in ANTENNAS:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--n", str(args.n), "--step", str(A)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step A {A} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        for line in got:
            rows.append(json.loads(line))
            print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
