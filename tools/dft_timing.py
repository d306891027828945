#!/usr/bin/env python3
"""Direct-Fourier prediction (gridhip_dft_predict_dev): device time per call and component-visibility terms per second at
    n = 10^6, C = 10^3, T = 1      n = 10^6, C = 10^3, T = 2 (with x)      n = 10^4, C = 10^5 (the sliced path)
the last both with the slices auto chooses and with "dft_slices" = 1.  Beside each: the same sum as a chunked fp64 torch
composition (torch.exp of the complex phase matrix times the flux vector, chunks of 2^24 terms), and the fp64 FMA rate
of the device as tools/micro/fma64_banks measures it (cycles per v_fma_f64, mode 0; build it first, see its head
comment - without the binary the column is left out), as FMA-equivalents per term.  Device events on torch's stream, warm-up
calls first, the median of --reps timed ones.
usage: python tools/dft_timing.py [--reps 20] [--warmup 3] [--out profiles/dft_n1e6.jsonl]"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
import torch  # noqa: E402

import gridhip  # noqa: E402

SHAPES = [(1_000_000, 1_000, 1), (1_000_000, 1_000, 2), (10_000, 100_000, 1)]


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


def torch_dft(comps, u, v, w, x, T, out, terms=1 << 24):
    """the same sum of point components as a torch composition, `terms` phase-matrix elements at a time"""
    l, m = comps[:, 0], comps[:, 1]
    r2 = l * l + m * m
    nm1 = -r2 / (1 + torch.sqrt(1 - r2))
    C_, n = comps.shape[0], u.shape[0]
    rows = max(1, terms // C_)
    for k0 in range(0, n, rows):
        s = slice(k0, min(n, k0 + rows))
        p = u[s, None] * l[None, :] + v[s, None] * m[None, :] + w[s, None] * nm1[None, :]
        ph = torch.exp(torch.complex(torch.zeros_like(p), (-2 * math.pi) * (p - torch.round(p))))
        if T == 1:
            out[s] = ph @ comps[:, 2].to(torch.complex128)
        else:
            flux = comps[None, :, 2] + x[s, None] * comps[None, :, 3]
            out[s] = (ph * flux).sum(dim=1)
    return out


def fma_rate(ctx, dev):
    """fp64 FMAs per second of the whole device from tools/micro/fma64_banks (mode 0: cycles per v_fma_f64 of one wave per
    SIMD, 64 lanes each) at the shader clock the library reads during a tile kernel (option "clock_khz"), or None - and a
    line on stderr - when the binary has not been built or the clock could not be read.  The micro-benchmark counts its
    cycles with s_memtime, the counter the library itself divides by s_memrealtime's fixed-rate one to get "clock_khz"
    (include/gridhip.h): both figures are in the same ticks, those of the shader clock."""
    import numpy as np
    exe = os.path.join(ROOT, "tools", "micro", "fma64_banks")
    if not os.path.exists(exe):
        print(f"{exe} has not been built: the FMA-equivalents column is left out", file=sys.stderr, flush=True)
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"mode 0 .*?([0-9.]+) cycles per instruction", out)
    if not m:
        print(f"{exe} printed no mode 0 line: the FMA-equivalents column is left out", file=sys.stderr, flush=True)
        return None
    rng = np.random.default_rng(0)  # a convgrid2 on the tap-reusing tile kernel, which stamps the clock
    N, W, Q, S, n = 256, 8, 8, 15, 200_000
    gcf = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ctx.convgrid2(gcf, np.zeros((N, N), dtype=np.complex128), (rng.uniform(-0.45, 0.45, n), rng.uniform(-0.45, 0.45, n), None),
                  rng.integers(0, W, n), rng.normal(size=n) + 0j)
    khz, cus = ctx.get_option("clock_khz"), torch.cuda.get_device_properties(dev).multi_processor_count
    r = {"cycles_per_fma64": float(m.group(1)), "clock_khz": khz, "compute_units": cus, "fma_per_s": None}
    if khz > 0:
        r["fma_per_s"] = cus * 4 * 64 / r["cycles_per_fma64"] * khz * 1e3
    else:
        print("the library read no shader clock: the FMA-equivalents column is left out", file=sys.stderr, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dft_n1e6.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0x9E3779B9)
    uni = lambda k, lo, hi: torch.rand(k, dtype=torch.float64, device=dev, generator=g) * (hi - lo) + lo  # noqa: E731
    ctx = gridhip.Context(0)
    fma = fma_rate(ctx, dev)
    head = {"device": torch.cuda.get_device_name(0), "fma64": fma}
    rows = []

    def rec(what, r, **extra):
        row = dict(head, what=what, **r, **extra)
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n, C_, T in SHAPES:
        u, v, w, x = uni(n, -2e4, 2e4), uni(n, -2e4, 2e4), uni(n, -2e4, 2e4), uni(n, -0.3, 0.3)
        comps = torch.zeros((C_, 10), dtype=torch.float64, device=dev)
        comps[:, 0], comps[:, 1] = uni(C_, -0.2, 0.2), uni(C_, -0.2, 0.2)
        comps[:, 2], comps[:, 3] = uni(C_, 0.5, 1.5), uni(C_, -0.5, 0.5)
        out, ref = (torch.empty(n, dtype=torch.complex128, device=dev) for _ in range(2))
        xs = x if T > 1 else None
        terms = float(n) * C_
        for forced in ((0,) if n >= 100_000 else (0, 1)):
            ctx.set_option("dft_slices", forced)
            fn = lambda: ctx.dft_predict((u, v, w), comps, x=xs, terms=T, out=out, stats=True)  # noqa: E731
            r = timed(fn, args.reps, args.warmup)
            S = int(fn()[1][3].item())
            rate = terms / (r["median_ms"] * 1e-3)
            auto_ms = r["median_ms"] if not forced else auto_ms
            rec(f"dft_predict_dev n {n} C {C_} T {T}" + (" dft_slices 1" if forced else ""), r, n=n, C=C_, T=T, slices=S,
                terms_per_s=rate, fma_equivalents_per_term=(fma["fma_per_s"] / rate if fma and fma["fma_per_s"] else None))
        ctx.set_option("dft_slices", 0)
        t = timed(lambda: torch_dft(comps, u, v, w, x, T, ref), max(3, args.reps // 4), 1)
        err = float((out - ref).abs().max() / comps[:, 2].abs().sum())
        rec(f"torch composition n {n} C {C_} T {T}", t, n=n, C=C_, T=T, terms_per_s=terms / (t["median_ms"] * 1e-3),
            over_dft_predict=t["median_ms"] / auto_ms, max_difference_of_flux=err)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
