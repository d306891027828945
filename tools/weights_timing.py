#!/usr/bin/env python3
"""The imaging weights at n = 1e6, 1e7 and 1e8 visibilities on N = 2400 (the driver's image size) and N = 4096, uniform
and Briggs weighting, each without and with data weights:
  native   ctx.weights on device tensors (stride 1, no taper): milliseconds per call, replayed from a captured graph of
           back-to-back calls between two device events, the median of the windows;
  torch    the same formula as an fp64 torch composition on the same device and inputs - the cell by floor arithmetic,
           bincount / index_add_ for the density, a gather, the elementwise weight - which is what a user writes without
           the library.  It is the yardstick, not the code under test; it computes the weights alone (no stats).
Next to each native figure the compulsory traffic of its passes at 6.29 TB/s (the copy rate the other tools use):
  pass 1   u, v (16 B) [+ s, 8 B] read, the cell code (8 B) written;
  pass 2   the cell code (8 B) [+ s, 8 B] read, w (8 B) written;
  cells    the density zeroed (4 or 8 B per cell) and, for Briggs, read once more;
the density's atomics and gathers are not counted (they are not compulsory bytes: they hit the caches or they do not).
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/weights_timing.py [--reps 10] [--out profiles/weights_timing.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE = 6.29e12
SIZES = [(2400, n) for n in (10 ** 6, 10 ** 7, 10 ** 8)] + [(4096, n) for n in (10 ** 6, 10 ** 7, 10 ** 8)]
SHAPE = {2400: (0.08, 30000), 4096: (0.128, 32000)}  # theta, lam with round(theta * lam) = N


def timed(torch, fn, reps, graph):
    """device milliseconds per fn() between two events around `inner` calls, the windows' median; inner is sized so that
    a window lasts about 20 ms.  graph: the inner calls are captured once and replayed."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    inner = max(1, min(100, int(20.0 / max(a.elapsed_time(b), 1e-3))))

    def window():
        for _ in range(inner):
            fn()
    run = window
    if graph:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn()  # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            window()
        torch.cuda.synchronize()
        run = g.replay
        run()
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms), "inner": inner,
            "graph": graph}


def composition(torch, N, lam, u, v, s, mode, robust):
    """the weights of the formula in fp64 torch (no taper, nothing flagged: s > 0 everywhere)"""
    fx = torch.floor((N // 2 + (u / lam) * N) + 0.5)
    fy = torch.floor((N // 2 + (v / lam) * N) + 0.5)
    ok = (fx >= 0) & (fy >= 0) & (fx < N) & (fy < N)
    c = torch.where(ok, fy * N + fx, torch.zeros_like(fx)).to(torch.int64)
    if s is None:
        D = torch.bincount(c, weights=ok.to(torch.float64), minlength=N * N)
        s = torch.ones_like(u)
    else:
        D = torch.zeros(N * N, dtype=torch.float64, device=u.device).index_add_(0, c, torch.where(ok, s, torch.zeros_like(s)))
    Dk = D[c]
    if mode == "uniform":
        w = s / Dk
    else:
        f2 = (5.0 * 10.0 ** -robust) ** 2 / ((D * D).sum() / D.sum())
        w = s / (1.0 + Dk * f2)
    return torch.where(ok, w, s)


def step(N, n, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    theta, lam = SHAPE[N]
    g = torch.Generator(device=dev).manual_seed(N + n % 1000)
    ctx = gridhip.Context(0)
    assert ctx.image_size(theta, lam) == N
    # a Gaussian core over a uniform disc of baselines, a few per cent beyond the grid's edge
    u = torch.where(torch.rand(n, device=dev, generator=g) < 0.5,
                    0.15 * torch.randn(n, dtype=torch.float64, device=dev, generator=g),
                    1.04 * (torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 0.5)) * lam
    v = torch.where(torch.rand(n, device=dev, generator=g) < 0.5,
                    0.15 * torch.randn(n, dtype=torch.float64, device=dev, generator=g),
                    1.04 * (torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 0.5)) * lam
    sw = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    out = torch.empty(n, dtype=torch.float64, device=dev)
    rows = []
    for mode in ("uniform", "briggs"):
        for given in (False, True):
            s = sw if given else None
            nat = timed(torch, lambda: ctx.weights(theta, lam, (u, v), mode, 0.5, 0.0, s, out=out), reps, True)
            w, st = ctx.weights(theta, lam, (u, v), mode, 0.5, 0.0, s)
            tor = timed(torch, lambda: composition(torch, N, lam, u, v, s, mode, 0.5), max(3, reps // 2), False)
            ref = composition(torch, N, lam, u, v, s, mode, 0.5)
            diff = ((w - ref).abs() / ref.abs()).max().item()
            del ref
            cell_b = (8 if given else 4) * N * N * (2 if mode == "briggs" else 1)
            bytes_ = n * ((16 + 8 + (8 if given else 0)) + (8 + 8 + (8 if given else 0))) + cell_b
            floor = bytes_ / COPY_RATE * 1e3
            rows.append({"N": N, "n": n, "mode": mode, "data_weights": given, "device": torch.cuda.get_device_name(0),
                         "native": nat, "torch": tor, "native_ms": nat["median_ms"], "torch_ms": tor["median_ms"],
                         "torch_over_native": tor["median_ms"] / nat["median_ms"], "compulsory_bytes": bytes_,
                         "floor_ms": floor, "fraction_of_floor": floor / nat["median_ms"],
                         "max_rel_diff_vs_torch": diff, "stats": st.cpu().tolist()})
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weights_timing.jsonl"))
    ap.add_argument("--step", metavar="N,n", help="run one size in this process (internal)")
    args = ap.parse_args()
    if args.step:
        N, n = (int(x) for x in args.step.split(","))
        for row in step(N, n, args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for N, n in SIZES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", f"{N},{n}"], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step N {N} n {n} ended with status {r.returncode}: nothing more is started", flush=True)
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
