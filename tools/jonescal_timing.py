#!/usr/bin/env python3
"""One iteration of the Jones solver and one apply_jones at a few (n, A, T), time-major, on the GPU and under no profiler:
  jonescal     ctx.jonescal (full mode) on device tensors with tol = 0 at niter = K and niter = 2 K: the difference of the two
               medians over K is one iteration (the streaming kernel plus the one-work-group update) without the prepare
               pass, the rotation and the chi^2 pass.  Events around eager calls, warm-up first, the median and the extremes
               of `reps` runs.
  apply_jones  ctx.apply_jones(inverse=True) with weights, out of place: 8 B + 64 B read, 64 B + 8 B written and the three
               index arrays, 168 B per visibility.
  torch        the same iteration composed of torch operations - gathers of the gains, batched 2x2 `matmul`, `index_add_`
               into [T * A] tables and a batched solve: the baseline tools/average_timing.py uses - and the same apply.
Next to each figure the bytes an iteration streams - 144 per visibility (key 8, s 8, V 64, M 64) - the time those bytes
take at 6.29 TB/s (the measured copy rate; the HBM peak is 8 TB/s), the ratio of the two, the LDS atomics (24 per
visibility) per second, and the shader clock the library read during a tile kernel just before ("clock_khz", 0: not read).
Every shape is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/jonescal_timing.py [--reps 7] [--out profiles/jonescal_timing.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE = 6.29e12
K = 4
SHAPES = [(1_440_000, 64, 16), (5_760_000, 64, 16), (5_760_000, 512, 16)]  # (n, A, T)
ITER_BYTES, APPLY_BYTES, ADDS = 144, 168, 24


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


def iteration(torch, solve, reps, n):
    t1, t2 = timed(torch, lambda: solve(K), reps), timed(torch, lambda: solve(2 * K), reps)
    it_ms = (t2["median_ms"] - t1["median_ms"]) / K
    spread = ((t2["max_ms"] - t1["min_ms"]) / K, (t2["min_ms"] - t1["max_ms"]) / K)
    floor_ms = ITER_BYTES * n / COPY_RATE * 1e3
    return {"solve_K": t1, "solve_2K": t2, "K": K, "iteration_ms": it_ms, "iteration_ms_spread": [min(spread), max(spread)],
            "bytes_per_vis": ITER_BYTES, "ms_at_copy_rate": floor_ms, "iteration_over_copy_rate": it_ms / floor_ms,
            "effective_GBps": ITER_BYTES * n / (it_ms * 1e-3) / 1e9, "lds_adds_per_ns": ADDS * n / (it_ms * 1e6)}


def shader_clock(ctx):
    """the shader clock in kHz the library reads during a tile kernel (option "clock_khz"; 0: it could not be read)"""
    import numpy as np
    rng = np.random.default_rng(0)
    N, W, Q, S, n = 256, 8, 8, 15, 200_000
    gcf = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ctx.convgrid2(gcf, np.zeros((N, N), dtype=np.complex128), (rng.uniform(-0.45, 0.45, n), rng.uniform(-0.45, 0.45, n), None),
                  rng.integers(0, W, n), rng.normal(size=n) + 0j)
    return ctx.get_option("clock_khz")


def torch_iteration(torch, V, M, s, p, q, t, A, T, G):
    """one full-mode iteration from G in torch operations: the sums by index_add_, G' = num den^-1 by a batched solve"""
    cells = T * A
    ip, iq = t * A + p, t * A + q
    Gf = G.reshape(cells, 2, 2)
    num, den = torch.zeros_like(Gf), torch.zeros_like(Gf)
    Z = torch.matmul(M, Gf[iq].mH)
    sZh = (s[:, None, None] * Z).mH
    num.index_add_(0, ip, torch.matmul(V, sZh))
    den.index_add_(0, ip, torch.matmul(Z, sZh))
    Z = torch.matmul(M.mH, Gf[ip].mH)
    sZh = (s[:, None, None] * Z).mH
    num.index_add_(0, iq, torch.matmul(V.mH, sZh))
    den.index_add_(0, iq, torch.matmul(Z, sZh))
    return torch.linalg.solve(den, num, left=False).reshape(T, A, 2, 2)  # X den = num


def torch_apply(torch, G, V, w, p, q, t, A):
    Gf = G.reshape(-1, 2, 2)
    inv, det = torch.linalg.inv(Gf), torch.linalg.det(Gf).abs()  # (of the T * A matrices, then gathered)
    ip, iq = t * A + p, t * A + q
    return torch.matmul(torch.matmul(inv[ip], V), inv[iq].mH), w * det[ip] * det[iq]


def step(n, A, T, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(A)
    ctx = gridhip.Context(0)
    khz = shader_clock(ctx)
    c128 = torch.complex128

    def mats(*shape):
        return torch.randn(*shape, 2, 2, dtype=c128, device=dev, generator=gen)
    a1 = torch.randint(0, A, (n,), device=dev, generator=gen)
    a2 = (a1 + torch.randint(1, A, (n,), device=dev, generator=gen)) % A
    slot = (torch.arange(n, device=dev) * T) // n  # time-major: T equal runs
    w = 0.5 + torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    M = mats(n)
    Gt = torch.eye(2, dtype=c128, device=dev) + 0.2 * mats(T, A)
    V = ctx.apply_jones(Gt, M, a1, a2, slot=slot, inverse=False)[0] + 0.05 * mats(n)
    g = torch.empty(T, A, 2, 2, dtype=c128, device=dev)
    eye = torch.eye(2, dtype=c128, device=dev).expand(T, A, 2, 2)

    def solve(niter):
        g.copy_(eye)
        return ctx.jonescal(V, M, a1, a2, A, slot=slot, nslots=T, weights=w, niter=niter, tol=0.0, gains=g)
    row = iteration(torch, solve, reps, n)
    stats = solve(2 * K)[1].cpu().tolist()
    lim = gridhip.jonescal_lds_antennas()
    table = A * 160
    group = 256 if 4 * (table + 64) <= 160 * 1024 else 512 if 2 * (table + 64) <= 160 * 1024 else 1024
    out, wout = torch.empty_like(V), torch.empty_like(w)
    ap = timed(torch, lambda: ctx.apply_jones(g, V, a1, a2, slot=slot, weights=w, out=out, weights_out=wout), reps)
    tit = timed(torch, lambda: torch_iteration(torch, V, M, w, a1, a2, slot, A, T, eye), reps)
    tap = timed(torch, lambda: torch_apply(torch, g, V, w, a1, a2, slot, A), reps)
    # the composition computes what the kernels compute: the apply with the solved gains, one iteration from the identity
    aerr = float((out - torch_apply(torch, g, V, w, a1, a2, slot, A)[0]).abs().max() / out.abs().max())
    g.copy_(eye)
    one = ctx.jonescal(V, M, a1, a2, A, slot=slot, nslots=T, weights=w, niter=1, tol=0.0, gains=g, refant=None)[0]
    err = float((one - torch_iteration(torch, V, M, w, a1, a2, slot, A, T, eye)).abs().max() / one.abs().max())
    ctx.close()
    return {"n": n, "A": A, "T": T, "device": torch.cuda.get_device_name(0), "clock_khz": khz,
            "path": "lds" if A <= lim else "global", "lds_bytes": table if A <= lim else 0,
            "work_group": group if A <= lim else 256, **row, "stats": stats,
            "apply": {**ap, "bytes_per_vis": APPLY_BYTES, "ms_at_copy_rate": APPLY_BYTES * n / COPY_RATE * 1e3,
                      "effective_GBps": APPLY_BYTES * n / (ap["median_ms"] * 1e-3) / 1e9},
            "torch_iteration": tit, "torch_apply": tap, "torch_over_iteration": tit["median_ms"] / row["iteration_ms"],
            "torch_over_apply": tap["median_ms"] / ap["median_ms"], "iteration_vs_torch_rel_err": err,
            "apply_vs_torch_rel_err": aerr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jonescal_timing.jsonl"))
    ap.add_argument("--step", metavar="n,A,T", help="run one shape in this process (internal)")
    args = ap.parse_args()
    if args.step:
        n, A, T = (int(x) for x in args.step.split(","))
        print("ROW " + json.dumps(step(n, A, T, args.reps)), flush=True)
        return 0
    rows = []
    for n, A, T in SHAPES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--step", f"{n},{A},{T}"], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step n {n} A {A} T {T} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
