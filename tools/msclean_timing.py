#!/usr/bin/env python3
"""Multi-scale CLEAN at N = 2400 (the driver's image size), gain 0.1, in one run on one device:
  setup     the set-up of ctx.msclean - the taps, the S (S + 1) / 2 - 1 cross-PSFs, the S - 1 smoothed residuals, the S
            tile tables and the first pick: a call with niter = 0;
  msclean   microseconds per iteration for S = 1, 3, 5 scales with patch 0 (the whole cross-PSF) and patch 64:
            (a call with niter = NITER minus the call with niter = 0) / NITER, enqueued eagerly;
  clean     ctx.clean's microseconds per iteration on the same inputs, measured the same way.
The expectation an iteration is written to: S Hogbom iterations, since slice t moves the bytes of one Hogbom iteration.
The measuring runs in one child process under `timeout`: if it fails, faults or runs out of time nothing more is started
on the device and no file is written.
usage: python tools/msclean_timing.py [--reps 5] [--out profiles/msclean_n2400.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, NITER, GAIN = 2400, 200, 0.1
SCALES = {1: [0.0], 3: [0.0, 4.0, 10.0], 5: [0.0, 2.0, 4.0, 8.0, 16.0]}
PATCHES = (0, 64)


def measure(reps):
    import torch
    import gridhip
    from clean_timing import inputs, timed
    dev = torch.device("cuda:0")
    psf, img = inputs(torch, dev)
    yy = torch.arange(N, device=dev, dtype=torch.float64) - N // 2
    blob = torch.exp(-0.5 * (yy[:, None] ** 2 + yy[None, :] ** 2) / 36.0)  # extended emission: wide scales get taken
    img = (img + torch.fft.ifft2(torch.fft.fft2(torch.fft.ifftshift(blob)) * torch.fft.fft2(torch.fft.ifftshift(psf))).real
           ).contiguous()
    res, model = img.clone(), torch.zeros_like(img)

    def reset():
        res.copy_(img)
        model.zero_()

    ctx = gridhip.Context(0)
    head = {"N": N, "niter": NITER, "gain": GAIN, "device": torch.cuda.get_device_name(0)}
    rows = []
    for patch in PATCHES:
        kw = dict(gain=GAIN, threshold=0.0, patch=patch, model=model)
        t0 = timed(torch, lambda: ctx.clean(res, psf, niter=0, **kw), reset, reps)
        t1 = timed(torch, lambda: ctx.clean(res, psf, niter=NITER, **kw), reset, reps)
        clean_us = (t1["median_ms"] - t0["median_ms"]) * 1e3 / NITER
        rows.append(dict(head, what="clean", patch=patch, niter0=t0, full=t1, us_per_iteration=clean_us))
        for S, scales in SCALES.items():
            t0 = timed(torch, lambda: ctx.msclean(res, psf, scales, niter=0, **kw), reset, reps)
            t1 = timed(torch, lambda: ctx.msclean(res, psf, scales, niter=NITER, **kw), reset, reps)
            _, _, stats = ctx.msclean(res, psf, scales, niter=NITER, **kw)
            us = (t1["median_ms"] - t0["median_ms"]) * 1e3 / NITER
            rows.append(dict(head, what="msclean", S=S, scales=scales, patch=patch, setup_ms=t0["median_ms"], niter0=t0,
                             full=t1, us_per_iteration=us, over_clean=us / clean_us, stats=stats.cpu().tolist()))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msclean_n2400.jsonl"))
    ap.add_argument("--child", action="store_true", help="measure in this process (internal)")
    args = ap.parse_args()
    if args.child:
        for row in measure(args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                        "--child"], stdout=subprocess.PIPE, text=True)
    got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
    if r.returncode != 0 or len(got) != len(PATCHES) * (1 + len(SCALES)):
        print(f"the measuring process ended with status {r.returncode} after {len(got)} rows: nothing is written", flush=True)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in got:
            print(line, flush=True)
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
