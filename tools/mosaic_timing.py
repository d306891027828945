#!/usr/bin/env python3
"""gridhip_mosaic_dev at a size a wide-field run has, on the GPU and under no profiler:
  mosaic   nf x nf overlapping feathered facets (gridhip.facet_grid, overlap 0.25) of Ns^2 cells onto 4096^2 cells, "cubic"
           and "bilinear", with the per-tile cull and without it (option "mosaic_cull" = 1): 4 x 4 facets of 1024^2 and 16 x 16
           facets of 256^2 - the same source cells, sixteen times the facets.
  torch    the composition torch offers: the positions formed by torch operations, `grid_sample` bilinear in fp64 per facet,
           the smoothstep window, a weighted accumulation and one division - F passes over the destination.
  floor    (F Ns^2 + Nd^2) 8 B, every source cell read and every destination cell written once, at 6.29 TB/s (the measured
           copy rate; the HBM peak is 8 TB/s).
Events on the stream around eager calls, a warm-up first, the median and the extremes of `reps` runs.  Beside the times the
largest difference between the bilinear mosaic and the composition (their interpolation is the same up to rounding).
Every case is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/mosaic_timing.py [--reps 7] [--out profiles/mosaic_timing.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE = 6.29e12
ND, THETA, OVERLAP = 4096, 0.2, 0.25
CASES = [(4, 1024), (16, 256)]  # (nf, Ns)


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


def torch_mosaic(torch, fac, theta_s, R, theta_d, Nd, inner, outer):
    """the bilinear mosaic out of torch operations: one grid_sample and one accumulation per facet"""
    F, Ns = fac.shape[0], fac.shape[1]
    h = float(Ns // 2)
    lc = theta_d * (torch.arange(Nd, device=fac.device, dtype=torch.float64) - Nd // 2) / Nd
    m, l = torch.meshgrid(lc, lc, indexing="ij")
    r2 = l * l + m * m
    live = r2 < 1.0
    n = torch.sqrt(torch.where(live, 1.0 - r2, torch.zeros_like(r2)))
    num, den = torch.zeros_like(l), torch.zeros_like(l)

    def feather(d):
        if outer == inner:
            return (d <= inner).to(torch.float64)
        t = ((outer - d) / (outer - inner)).clamp(0.0, 1.0)
        return t * t * (3.0 - 2.0 * t)
    for f in range(F):
        r = R[f]
        fx = (r[0] * l + r[1] * m + r[2] * n) * Ns / theta_s + h
        fy = (r[3] * l + r[4] * m + r[5] * n) * Ns / theta_s + h
        w = feather((fx - h).abs()) * feather((fy - h).abs())
        ok = live & ((r[6] * l + r[7] * m + r[8] * n) > 0) & (fx >= 0) & (fx < Ns - 1) & (fy >= 0) & (fy < Ns - 1)
        grid = torch.stack((2.0 * fx / (Ns - 1) - 1.0, 2.0 * fy / (Ns - 1) - 1.0), dim=-1)[None]
        v = torch.nn.functional.grid_sample(fac[f][None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
        w = torch.where(ok, w, torch.zeros_like(w))
        num += w * v
        den += w
    return torch.where(den > 0, num / den, torch.full_like(num, float("nan")))


def step(nf, Ns, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(nf)
    ctx = gridhip.Context(0)
    centres, R, theta_f, window = gridhip.facet_grid(THETA, nf, OVERLAP, Ns)
    F = nf * nf
    fac = torch.randn(F, Ns, Ns, dtype=torch.float64, device=dev, generator=gen)
    dR = torch.from_numpy(R).to(dev)
    out = torch.empty(ND, ND, dtype=torch.float64, device=dev)
    floor_ms = (F * Ns * Ns + ND * ND) * 8 / COPY_RATE * 1e3
    row = {"nf": nf, "F": F, "Ns": Ns, "Nd": ND, "theta": THETA, "theta_f": theta_f, "window": list(window),
           "device": torch.cuda.get_device_name(0), "bytes": (F * Ns * Ns + ND * ND) * 8, "ms_at_copy_rate": floor_ms}
    for kind in ("cubic", "bilinear"):
        for cull in (1, 0):
            ctx.set_option("mosaic_cull", 0 if cull else 1)
            t = timed(torch, lambda: ctx.mosaic(fac, theta_f, dR, THETA, ND, kind, window=window, out=out), reps)
            row[f"{kind}_{'cull' if cull else 'all_facets'}"] = {**t, "over_copy_rate": t["median_ms"] / floor_ms}
        ctx.set_option("mosaic_cull", 0)
        row[f"{kind}_cull_gain"] = row[f"{kind}_all_facets"]["median_ms"] / row[f"{kind}_cull"]["median_ms"]
    _, stats = ctx.mosaic(fac, theta_f, dR, THETA, ND, "bilinear", window=window, out=out, stats=True)
    row["stats"] = stats.cpu().tolist()
    tt = timed(torch, lambda: torch_mosaic(torch, fac, theta_f, R, THETA, ND, *window), max(3, reps // 2))
    ref = torch_mosaic(torch, fac, theta_f, R, THETA, ND, *window)
    both = torch.isfinite(out) & torch.isfinite(ref)
    row["torch"] = tt
    row["torch_over_bilinear"] = tt["median_ms"] / row["bilinear_cull"]["median_ms"]
    row["torch_over_cubic"] = tt["median_ms"] / row["cubic_cull"]["median_ms"]
    row["bilinear_vs_torch_max_abs"] = float((out - ref)[both].abs().max())
    row["cells_finite_in_both"] = int(both.sum())
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mosaic_timing.jsonl"))
    ap.add_argument("--step", metavar="nf,Ns", help="run one case in this process (internal)")
    args = ap.parse_args()
    if args.step:
        nf, Ns = (int(x) for x in args.step.split(","))
        print("ROW " + json.dumps(step(nf, Ns, args.reps)), flush=True)
        return 0
    rows = []
    for nf, Ns in CASES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--step", f"{nf},{Ns}"], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step nf {nf} Ns {Ns} ended with status {r.returncode}: nothing more is started", flush=True)
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
