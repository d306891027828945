#!/usr/bin/env python3
"""Continuum subtraction against its two yardsticks, device events, the median of `reps` runs, all in one process per
channel count:
  device    ctx.contsub on R = 2^20 spectra of C = 64 and C = 512 channels, complex and real, channel-innermost (axis -1,
            through LDS) and channel-outermost (axis 0, straight from global memory), degree 1 and 3, without rounds and
            with nsigma = 3, niter = 3, each as a captured graph that is replayed.  The spectra are a linear continuum
            plus unit noise plus a line of 4 channels, so the rounds have something to clip;
  torch_sub torch.sub(a, b, out=c) over the same bytes: two reads and one write of the data, what a call without
            rounds moves at the least - the floor of a memory-bound job;
  torch_fit the same fit through torch operations, eagerly: the Vandermonde matrix of the Chebyshev basis, per row the
            normal matrix einsum("rc,cj,ck->rjk") over the participants and the right-hand side, torch.linalg.solve on
            the R systems, the model by a matrix product, and for rounds the residual power against nsigma^2 times the
            row's mean.  Not the same bits: a baseline for the time only.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/contsub_timing.py [--reps 5] [--rows 1048576] [--out profiles/contsub_timing.jsonl]"""
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

STEPS = [("64", 420), ("512", 600)]
NSIGMA, NITER = 3.0, 3


def spectra(torch, dev, R, C, cplx):
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.linspace(-1.0, 1.0, C, dtype=torch.float64, device=dev)
    re = torch.randn((R, C), dtype=torch.float64, device=dev, generator=g)
    a = torch.randn((R, 2), dtype=torch.float64, device=dev, generator=g)
    re += a[:, :1] + a[:, 1:] * x[None, :]
    re[:, C // 3:C // 3 + 4] += 8.0
    if not cplx:
        return re, x
    im = torch.randn((R, C), dtype=torch.float64, device=dev, generator=g)
    return torch.complex(re, im), x


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


def torch_fit(torch, data, x, degree, niter):
    """[R][C] -> data minus the fitted continuum, by torch operations"""
    C = x.shape[0]
    T = [torch.ones_like(x), x]
    for p in range(1, degree):
        T.append(2.0 * x * T[p] - T[p - 1])
    V = torch.stack(T[:degree + 1], dim=1)                       # [C][D + 1]
    part = torch.ones(data.shape, dtype=torch.float64, device=data.device)
    VV = (V[:, :, None] * V[:, None, :]).reshape(C, -1)          # [C][(D + 1)^2]
    for rnd in range(niter + 1):
        A = (part @ VV).reshape(-1, degree + 1, degree + 1)      # einsum("rc,cj,ck->rjk")
        b = (part * data) @ V.to(data.dtype)                     # einsum("rc,cj->rj")
        coef = torch.linalg.solve(A.to(data.dtype), b)
        res = data - coef @ V.to(data.dtype).T
        if rnd == niter:
            return res
        q = part * (res.real * res.real + res.imag * res.imag if res.is_complex() else res * res)
        qbar = q.sum(dim=1) / part.sum(dim=1)
        part = part * (q <= (NSIGMA * NSIGMA) * qbar[:, None]).to(torch.float64)


def emit(row):
    print("ROW " + json.dumps(row), flush=True)


def step(what, reps, R):
    import torch
    import gridhip
    from noise_timing import replayed
    dev = torch.device("cuda:0")
    C = int(what)
    ctx = gridhip.Context(0)
    rows_, chunk = gridhip.contsub_tile()
    for cplx in (True, False):
        data, x = spectra(torch, dev, R, C, cplx)
        nbytes = data.numel() * data.element_size()
        base = {"device": torch.cuda.get_device_name(0), "R": R, "C": C, "dtype": str(data.dtype).replace("torch.", ""),
                "data_bytes": nbytes}
        other, out = torch.ones_like(data), torch.empty_like(data)
        r = timed(torch, lambda: torch.sub(data, other, out=out), reps)
        emit(dict(base, what="torch_sub", GBps=3 * nbytes / r["median_ms"] / 1e6, **r))
        del other
        for axis in (-1, 0):
            d = data if axis == -1 else data.T.contiguous()
            o = out.view(d.shape)
            for degree in (1, 3):
                for niter in (0, NITER):
                    kw = dict(axis=axis, degree=degree, nsigma=NSIGMA if niter else 0.0, niter=niter, out=o)
                    res = ctx.contsub(d, x, **kw)
                    st = [float(v) for v in res[4].tolist()]
                    r = replayed(torch, lambda: ctx.contsub(d, x, **kw), lambda: None, reps)
                    emit(dict(base, what="contsub_dev", axis=axis, degree=degree, niter=niter, tile=[rows_, chunk], stats=st,
                              GBps=3 * nbytes / r["median_ms"] / 1e6, **r))
                    del res
            del d, o
        for degree in (1, 3):
            for niter in (0, NITER):
                r = timed(torch, lambda: torch_fit(torch, data, x, degree, niter), max(2, reps // 2))
                emit(dict(base, what="torch_fit", degree=degree, niter=niter, **r))
        del data, out
        torch.cuda.empty_cache()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contsub_timing.jsonl"))
    ap.add_argument("--step", help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        step(args.step, args.reps, args.rows)
        return 0
    print(f"R = {args.rows}, reps = {args.reps}", flush=True)
    rows = []
    for what, limit in STEPS:
        r = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                              str(args.reps), "--rows", str(args.rows), "--step", what], stdout=subprocess.PIPE, text=True)
        got = []
        for line in r.stdout:  # (every row as it comes)
            if line.startswith("ROW "):
                got.append(line[4:].strip())
                print(got[-1], flush=True)
        if r.wait() != 0 or not got:
            print(f"step C = {what} ended with status {r.returncode}: nothing more is started", flush=True)
            break
        rows += [json.loads(x) for x in got]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0 if len({r["C"] for r in rows}) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
