#!/usr/bin/env python3
"""RM synthesis and RM-CLEAN against torch, device events after a warm-up, the median of `reps` runs, at M = 1024^2 lines
of sight, C = 64 channels, J = 256 depths (a cube of 4.3 GB); two Faraday-thin components and noise per line of sight:
  synth     ctx.rmsynth as a captured graph that is replayed (Q and U as the two real cubes they are);
  matmul    torch.matmul of the same complex128 product E^T [J x C] . P [C x M], once with P given and once with the copy
            of Q and U into the interleaved complex P inside the timed window;
  clean     ctx.rmclean at niter = 100, threshold 0 (every line of sight takes its 100 components), the two ways of
            reading the cube - every wave its own line of sight directly, or a work-group's four through LDS (option
            "rm_stage") - alternating in one process; and at a level of 5 sigma, where the loops differ in length;
  torch     the same 100 minor cycles for all lines of sight at once: |F|^2, argmax over the depths, a gather of the peak,
            a gather of the shifted RMSF and the subtraction.  Not the same bits; a baseline for the time only.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/rm_timing.py [--reps 5] [--m 1048576] [--out profiles/rm_timing.jsonl]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

C_, J = 64, 256
NITER, GAIN, SIGMA = 100, 0.1, 0.02
STEPS = [("synth", 300), ("matmul", 300), ("clean", 400), ("torch", 400)]


def grid():
    fwhm = 2.0 * math.sqrt(3.0) / 0.06
    dphi = fwhm / 4.0
    return -(J - 1) / 2 * dphi, dphi, fwhm


def sky(torch, dev, M):
    """lam2 [C], Q, U [C][M]: two components on grid depths and Gaussian noise per line of sight"""
    g = torch.Generator(device=dev).manual_seed(5)
    phi0, dphi, _ = grid()
    lam2 = torch.linspace(0.03, 0.09, C_, dtype=torch.float64, device=dev)
    P = SIGMA * torch.complex(torch.randn((C_, M), dtype=torch.float64, device=dev, generator=g),
                              torch.randn((C_, M), dtype=torch.float64, device=dev, generator=g))
    for _ in range(2):
        depth = phi0 + dphi * torch.randint(0, J, (M,), device=dev, generator=g).to(torch.float64)
        amp = torch.polar(0.5 + torch.rand(M, dtype=torch.float64, device=dev, generator=g),
                          2 * math.pi * torch.rand(M, dtype=torch.float64, device=dev, generator=g))
        angle = 2.0 * lam2[:, None] * depth[None, :]
        P += amp[None, :] * torch.polar(torch.ones_like(angle), angle)
    return lam2, P.real.contiguous(), P.imag.contiguous()


def timed(torch, work, reps, reset=lambda: None):
    reset()
    work()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        work()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def torch_clean(torch, cube, R, niter):
    Jn, M = cube.shape
    jj = torch.arange(Jn, device=cube.device)[:, None] + (Jn - 1)
    cols = torch.arange(M, device=cube.device)
    model = torch.zeros_like(cube)
    for _ in range(niter):
        k = (cube.real * cube.real + cube.imag * cube.imag).argmax(dim=0)
        f = GAIN * cube[k, cols]
        model[k, cols] += f
        cube -= f[None, :] * R[jj - k[None, :]]
    return model


def step(what, reps, M):
    import torch
    import gridhip
    from noise_timing import replayed
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "M": M, "C": C_, "J": J, "cube_GB": round(J * M * 16 / 1e9, 2)}
    phi0, dphi, fwhm = grid()
    lam2, Q, U = sky(torch, dev, M)
    ctx = gridhip.Context(0)
    tab = ctx.rm_tables(lam2, (phi0, dphi, J), fwhm=fwhm)
    nE = C_ * J
    E = torch.view_as_complex(tab[16:16 + 2 * nE].reshape(C_, J, 2))
    R = torch.view_as_complex(tab[16 + 2 * nE:16 + 2 * nE + 2 * (2 * J - 1)].reshape(2 * J - 1, 2))
    rows = []
    if what == "synth":
        out = torch.empty((J, M), dtype=torch.complex128, device=dev)
        res = ctx.rmsynth(Q, U, tab, out=out)
        r = replayed(torch, lambda: ctx.rmsynth(Q, U, tab, out=out), lambda: None, reps)
        flop = 8.0 * J * C_ * M
        rows.append(dict(base, what="rmsynth_dev", case="Q and U as two real cubes", tile=list(gridhip.rm_tile()),
                         stats=res[1].tolist(), fp64_instr_per_s=flop / (r["median_ms"] * 1e-3), **r))
    elif what == "matmul":
        Et = E.t().contiguous()
        P = torch.complex(Q, U)
        out = torch.empty((J, M), dtype=torch.complex128, device=dev)
        rows.append(dict(base, what="matmul", case="P given", **timed(torch, lambda: torch.matmul(Et, P, out=out), reps)))
        del P
        rows.append(dict(base, what="matmul", case="with the copy of Q, U into P",
                         **timed(torch, lambda: torch.matmul(Et, torch.complex(Q, U), out=out), reps)))
        ours = ctx.rmsynth(Q, U, tab)[0]
        rows[-1]["max_abs_diff_to_rmsynth"] = float((ours - out).abs().max())
    elif what == "clean":
        first = ctx.rmsynth(Q, U, tab)[0]
        del Q, U
        cube, model = torch.empty_like(first), torch.empty_like(first)
        noise = torch.tensor([SIGMA / math.sqrt(C_)], dtype=torch.float64, device=dev)  # the noise of F

        def reset():
            cube.copy_(first)
            model.zero_()
        for name, kw in (("niter 100, level 0", dict(threshold=0.0)), ("niter 100, level 5 sigma", dict(nsigma=5.0, noise=noise))):
            ms, stats = {0: [], 1: []}, None
            for rep in range(reps + 1):  # (the first pair is the warm-up; the two variants alternate)
                for stage in (0, 1):
                    ctx.set_option("rm_stage", stage)
                    reset()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    res = ctx.rmclean(cube, tab, gain=GAIN, niter=NITER, model=model, **kw)
                    b.record()
                    torch.cuda.synchronize()
                    if rep:
                        ms[stage].append(a.elapsed_time(b))
                    stats = res[3].tolist()
            ctx.set_option("rm_stage", 0)
            for stage, label in ((0, "direct"), (1, "through LDS")):
                rows.append(dict(base, what="rmclean_dev", case=name, cube_access=label, stats=stats,
                                 median_ms=statistics.median(ms[stage]), min_ms=min(ms[stage]), max_ms=max(ms[stage]), reps=reps))
    else:
        first = ctx.rmsynth(Q, U, tab)[0]
        del Q, U
        cube = torch.empty_like(first)
        torch_clean(torch, cube.copy_(first), R, 2)
        r = timed(torch, lambda: torch_clean(torch, cube, R, NITER), max(1, min(reps, 2)), reset=lambda: cube.copy_(first))
        rows.append(dict(base, what="torch", case="niter 100: argmax, gather, shifted-RMSF gather, subtract", **r))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, default=1024 * 1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rm_timing.jsonl"))
    ap.add_argument("--step", help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(args.step, args.reps, args.m):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for what, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--m", str(args.m), "--step", what], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} ended with status {r.returncode}: nothing more is started", flush=True)
            break
        rows += [json.loads(x) for x in got]
        print("\n".join(got), flush=True)
    access = {}
    for r in rows:
        if r["what"] == "rmclean_dev":
            access.setdefault(r["case"], {})[r["cube_access"]] = r["median_ms"]
    if access and all(len(a) == 2 for a in access.values()):  # the winner per case: loops of one length, loops that differ
        rows.append({"what": "rmclean_cube_access", "median_ms": access,
                     "winner": {case: min(a, key=a.get) for case, a in access.items()}})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0 if len({r["what"] for r in rows}) >= 5 else 1


if __name__ == "__main__":
    sys.exit(main())
