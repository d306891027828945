#!/usr/bin/env python3
"""One StEFCal iteration of the gain solver at n = 1e7 and 1e8 visibilities, A = 512 antennas, T = 64 solution intervals,
time-major:
  native   ctx.gaincal on device tensors with tol = 0 at niter = K and niter = 2 K: the difference of the two medians
           over K is one iteration (the streaming kernel plus the one-work-group update) without the prepare pass, the
           rotation and the chi^2 pass; the whole solves are reported too.  Events around eager calls (a solve is 2 K + 6
           launches of a millisecond each at these sizes: launch overhead does not show), warm-up first, the median and the
           extremes of `reps` runs.
  torch    the same iteration written as an fp64 torch composition on the same X, Y and indices - gathers of the gains,
           index_add_ into the (T A) table, the division - which is what a user writes without the library.  It is the
           yardstick, not the code under test.
Next to the native figure the effective rate against the 32 B per visibility an iteration streams (X 16, Y 8, key 8), and
that rate as a fraction of 6.29 TB/s (the copy rate the other tools use) and of the 8 TB/s HBM peak.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/gaincal_timing.py [--reps 7] [--out profiles/gaincal_n1e8.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE, HBM_PEAK = 6.29e12, 8.0e12
A, T, K = 512, 64, 4
SIZES = [10 ** 7, 10 ** 8]


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


def torch_iteration(torch, X, Y, ip, iq, g, cells):
    """g' = num / den of one iteration from g (flat [T A] complex) - no averaging, no rel: the sums and the division"""
    gp, gq = g[ip], g[iq]
    num = torch.zeros(cells, 2, dtype=torch.float64, device=g.device)
    num.index_add_(0, ip, torch.view_as_real(X * gq)).index_add_(0, iq, torch.view_as_real(X.conj() * gp))
    den = torch.zeros(cells, dtype=torch.float64, device=g.device)
    den.index_add_(0, ip, Y * (gq.real ** 2 + gq.imag ** 2)).index_add_(0, iq, Y * (gp.real ** 2 + gp.imag ** 2))
    ok = den > 0
    return torch.where(ok, torch.view_as_complex(num) / torch.where(ok, den, torch.ones_like(den)), g)


def step(n, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    ctx = gridhip.Context(0)
    a1 = torch.randint(0, A, (n,), device=dev, generator=gen)
    a2 = (a1 + torch.randint(1, A, (n,), device=dev, generator=gen)) % A
    slot = (torch.arange(n, device=dev) * T) // n  # time-major: T equal runs
    M = torch.randn(n, dtype=torch.complex128, device=dev, generator=gen) + 3
    gt = (1 + 0.2 * torch.randn(T, A, dtype=torch.float64, device=dev, generator=gen)) * torch.exp(
        1j * (2 * torch.rand(T, A, dtype=torch.float64, device=dev, generator=gen) - 1))
    V = gt[slot, a1] * M * gt[slot, a2].conj() + 0.1 * torch.randn(n, dtype=torch.complex128, device=dev, generator=gen)
    g = torch.ones(T, A, dtype=torch.complex128, device=dev)

    def solve(niter):
        g.fill_(1.0)
        return ctx.gaincal(V, M, a1, a2, A, slot=slot, nslots=T, niter=niter, tol=0.0, gains=g)
    t1, t2 = timed(torch, lambda: solve(K), reps), timed(torch, lambda: solve(2 * K), reps)
    stats = solve(2 * K)[1].cpu().tolist()
    it_ms = (t2["median_ms"] - t1["median_ms"]) / K
    spread = ((t2["max_ms"] - t1["min_ms"]) / K, (t2["min_ms"] - t1["max_ms"]) / K)
    rate = 32.0 * n / (it_ms * 1e-3)
    # the yardstick, on the same X, Y and flat indices, from g = 1; its first iterate against the library's
    X, Y = V * M.conj(), M.real ** 2 + M.imag ** 2
    ip, iq = slot * A + a1, slot * A + a2
    g1 = torch.ones(T * A, dtype=torch.complex128, device=dev)
    tor = timed(torch, lambda: torch_iteration(torch, X, Y, ip, iq, g1, T * A), max(3, reps // 2))
    g.fill_(1.0)
    lib1 = ctx.gaincal(V, M, a1, a2, A, slot=slot, nslots=T, niter=1, tol=0.0, refant=None, gains=g)[0].reshape(-1)
    diff = ((lib1 - torch_iteration(torch, X, Y, ip, iq, g1, T * A)).abs().max() / lib1.abs().max()).item()
    row = {"n": n, "A": A, "T": T, "device": torch.cuda.get_device_name(0), "solve_K": t1, "solve_2K": t2, "K": K,
           "iteration_ms": it_ms, "iteration_ms_spread": [min(spread), max(spread)], "bytes_per_vis": 32,
           "effective_GBps": rate / 1e9, "fraction_of_copy_rate": rate / COPY_RATE, "fraction_of_hbm_peak": rate / HBM_PEAK,
           "torch": tor, "torch_iteration_ms": tor["median_ms"], "torch_over_native": tor["median_ms"] / it_ms,
           "max_rel_diff_vs_torch": diff, "stats": stats}
    ctx.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaincal_n1e8.jsonl"))
    ap.add_argument("--step", metavar="n", help="run one size in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(int(args.step), args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for n in SIZES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", str(n)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step n {n} ended with status {r.returncode}: nothing more is started", flush=True)
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
