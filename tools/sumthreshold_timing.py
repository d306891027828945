#!/usr/bin/env python3
"""Time-frequency flagging against a torch composition, device events, the median of `reps` runs:
  device    ctx.sumthreshold on a cube of B x T x F = 64 x 512 x 512 samples (1.7 x 10^7: 64 baselines, 512 time steps,
            512 channels) of noise with a burst, a line and spikes, as a captured graph that is replayed: the default call
            (7 stages, 2 rounds, SIR both ways) in both orders, and the calls that take it apart - niter = 0 without SIR
            (front pass, counts, write-out), niter = 0 with SIR along frequency and along time, one round with 1 stage (front
            pass + select + 1 stage) and one round with 7 stages.  The differences say which of front pass, select, stages
            and SIR dominates;
  torch     the same cube through torch operations, eagerly: the amplitude, per baseline torch.median and the MAD, for every
            window length cumsum window sums and counts along frequency and time, the hits spread with a second cumsum, one
            round; then the SIR operator with cumsum, cummin and a flipped cummax.  Not the same bits (cumsum is no doubling
            tree): a baseline for the time only.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/sumthreshold_timing.py [--reps 10] [--out profiles/sumthreshold_timing.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

B, T, F = 64, 512, 512
STEPS = [("device", 300), ("torch", 300)]
LEVELS = [6.0 / 1.5 ** k for k in range(7)]


def cube(torch, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    vis = torch.complex(torch.randn((B, T, F), dtype=torch.float64, device=dev, generator=g),
                        torch.randn((B, T, F), dtype=torch.float64, device=dev, generator=g))
    add = torch.zeros((B, T, F), dtype=torch.float64, device=dev)
    add[1::4, 100:104, :] += 1.5
    add[2::4, :, 50] += 1.0
    add[:, 40::97, 70::89] += 12.0
    amp = vis.abs()
    vis = vis * ((amp + add) / amp)
    wt = torch.ones((B, T, F), dtype=torch.float64, device=dev)
    wt[0, :, 100] = 0.0
    return vis, wt


def window_hits(torch, x, c, chi, M, dim):
    """samples hit by a window of M along dim: window sums by cumsum, the hits spread by a cumsum of the hit windows"""
    L = x.shape[dim]
    if M > L:
        return torch.zeros_like(c, dtype=torch.bool)
    zero =lambda a: torch.zeros([1 if i == dim else s for i, s in enumerate(a.shape)], dtype=a.dtype, device=a.device)  # noqa: E731
    cs, cc = torch.cat([zero(x), x.cumsum(dim)], dim), torch.cat([zero(c), c.cumsum(dim)], dim)
    S = cs.narrow(dim, M, L - M + 1) - cs.narrow(dim, 0, L - M + 1)
    C = cc.narrow(dim, M, L - M + 1) - cc.narrow(dim, 0, L - M + 1)
    win = ((C > 0) & (S > chi * C)).to(torch.int32)
    # sample i is hit when a window in [i - M + 1, i] is: pad the windows to L + M and difference their cumsum
    shape = list(x.shape)
    shape[dim] = M
    wz = torch.zeros(shape, dtype=torch.int32, device=x.device)
    acc = torch.cat([wz, win, wz[tuple(slice(0, M - 1) if i == dim else slice(None) for i in range(3))]], dim).cumsum(dim)
    return (acc.narrow(dim, M, L) - acc.narrow(dim, 0, L)) > 0


def torch_round(torch, vis, wt):
    a = torch.sqrt(vis.real * vis.real + vis.imag * vis.imag)
    part = (wt > 0) & torch.isfinite(a)
    flat = torch.where(part, a, torch.full_like(a, float("nan"))).reshape(B, -1)
    med = torch.nanmedian(flat, dim=1).values
    mad = torch.nanmedian((flat - med[:, None]).abs(), dim=1).values
    sigma = (1.4826 * mad)[:, None, None]
    e = a - med[:, None, None]
    flags = torch.zeros_like(part)
    for k, level in enumerate(LEVELS):
        x = torch.where(part, e, torch.zeros_like(e))
        c = part.to(torch.float64)
        hit = window_hits(torch, x, c, level * sigma, 1 << k, 2) | window_hits(torch, x, c, level * sigma, 1 << k, 1)
        new = hit & part
        flags |= new
        part = part & ~new
    return flags, part


def torch_sir(torch, flags, part, eta, dim):
    q = int(round(eta * 2 ** 20))
    w = torch.where(flags, q, torch.where(part, q - (1 << 20), 0)).to(torch.int64)
    P = w.cumsum(dim)
    lo = torch.cummin(P - w, dim).values.clamp(max=0)
    hi = torch.cummax(P.flip(dim), dim).values.flip(dim)
    return flags | (part & (hi - lo >= 0))


def timed(torch, work, reps):
    work()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        work()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def step(what, reps):
    import torch
    import gridhip
    from noise_timing import replayed
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "F": F, "n": B * T * F}
    vis, wt = cube(torch, dev)
    rows = []
    if what == "device":
        ctx = gridhip.Context(0)
        out = torch.empty_like(wt)
        tt, tf = gridhip.sumthreshold_tile()
        cases = [("default", "btf", dict()), ("default", "tbf", dict()),
                 ("niter 0, no SIR", "btf", dict(niter=0, eta=(0, 0))), ("niter 0, SIR along f", "btf", dict(niter=0, eta=(0.2, 0))),
                 ("niter 0, SIR along t", "btf", dict(niter=0, eta=(0, 0.2))),
                 ("1 round, 1 stage, no SIR", "btf", dict(niter=1, nlevels=1, eta=(0, 0))),
                 ("1 round, 7 stages, no SIR", "btf", dict(niter=1, eta=(0, 0))),
                 ("1 round, 7 stages, no SIR", "tbf", dict(niter=1, eta=(0, 0)))]
        for name, order, kw in cases:
            v, w, o = (x if order == "btf" else x.transpose(0, 1).contiguous() for x in (vis, wt, out))
            res = ctx.sumthreshold(v, weights=w, order=order, out=o, **kw)
            r = replayed(torch, lambda: ctx.sumthreshold(v, weights=w, order=order, out=o, **kw), lambda: None, reps)
            rows.append(dict(base, what="sumthreshold_dev", case=name, order=order, tile=[tt, tf],
                             stats=[float(x) for x in res[3].tolist()], **r))
        ctx.close()
    else:
        flags, part = torch_round(torch, vis, wt)
        r = timed(torch, lambda: torch_round(torch, vis, wt), reps)
        rows.append(dict(base, what="torch", case="1 round, 7 stages (cumsum windows, nanmedian)", flagged=int(flags.sum()), **r))
        r = timed(torch, lambda: torch_sir(torch, torch_sir(torch, flags, part, 0.2, 2), part, 0.2, 1), reps)
        rows.append(dict(base, what="torch", case="SIR along f and t (cumsum, cummin, cummax)", **r))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumthreshold_timing.jsonl"))
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
    return 0 if len({r["what"] for r in rows}) >= 2 else 1


if __name__ == "__main__":
    sys.exit(main())
