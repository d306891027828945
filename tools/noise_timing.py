#!/usr/bin/env python3
"""image_stats, masked clean and the noise-aware loop at N = 2400 (the driver's image size), device events, the median
of 20 replays of a captured graph:
  stats     ctx.image_stats on a Gaussian-noise image - whose top key digits fall into a handful of bins, the worst case
            for the LDS atomics - and on an image of keys spread evenly, for the 13-bit digit (5 + 5 passes) and the 8-bit
            one (8 + 8, context option "noise_bits"); per pass = the call / the passes, beside the time the HBM roofline
            gives for reading N^2 x 8 B once at 6.29 TB/s;
  clean     microseconds per iteration of ctx.clean: the plain form, the _auto form without a mask and with one
            (expected: one byte per cell on top of 24);
  loop      Imager.deconvolve against the same call with nsigma (the _auto loop): the difference is the cost of knowing
            the noise.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/noise_timing.py [--reps 20] [--out profiles/noise_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, COPY_RATE = 2400, 6.29e12
STEPS = [("stats", 240), ("clean", 240), ("loop", 300)]


def replayed(torch, work, reset, reps):
    """device milliseconds of a replay of work() captured into a graph: `reps` times after the warm-up"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        reset()
        work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        work()
    torch.cuda.synchronize()
    ms = []
    for rep in range(reps + 1):
        reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def step(what, reps):
    import torch
    import gridhip
    import clean_timing
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    rows = []
    base = {"N": N, "device": torch.cuda.get_device_name(0)}
    if what == "stats":
        g = torch.Generator(device=dev).manual_seed(1)
        noise = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
        spread = torch.randint(-2 ** 62, 2 ** 62, (N, N), dtype=torch.int64, device=dev, generator=g).view(torch.float64)
        spread = torch.nan_to_num(spread, nan=1.0, posinf=2.0, neginf=-2.0)
        floor = N * N * 8 / COPY_RATE * 1e6
        for bits in (13, 8):
            ctx.set_option("noise_bits", bits)
            passes = 2 * ((64 + bits - 1) // bits)
            for name, img in (("gaussian noise", noise), ("spread keys", spread)):
                r = replayed(torch, lambda: ctx.image_stats(img), lambda: None, reps)
                rows.append(dict(base, what="image_stats", image=name, digit_bits=bits, passes=passes, launches=1 + 2 * passes,
                                 **r, us_per_pass=r["median_ms"] * 1e3 / passes, roofline_us_per_pass=floor,
                                 roofline_is="N^2 x 8 B once at 6.29 TB/s"))
        ctx.set_option("noise_bits", 0)
    elif what == "clean":
        niter = 200
        psf, img = clean_timing.inputs(torch, dev)
        res, model = img.clone(), torch.zeros_like(img)
        ones = torch.ones((N, N), dtype=torch.uint8, device=dev)

        def reset():
            res.copy_(img)
            model.zero_()
        for name, kw in (("plain", {}), ("auto, no mask", dict(peak_frac=1e-9)), ("auto, mask", dict(mask=ones))):
            r = replayed(torch, lambda: ctx.clean(res, psf, gain=0.1, niter=niter, model=model, **kw), reset, reps)
            rows.append(dict(base, what="clean", form=name, niter=niter, patch=0, **r,
                             us_per_iteration=r["median_ms"] * 1e3 / niter,
                             floor_us=(25.0 if "mask" in kw else 24.0) * N * N / COPY_RATE * 1e6))
    else:
        nvis, lam, theta, nmajor, niter = 200000, 24000, 0.1, 3, 50
        g = torch.Generator(device=dev).manual_seed(2)
        u, v = ((torch.rand(nvis, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.6 * lam for _ in range(2))
        w = torch.zeros(nvis, dtype=torch.float64, device=dev)
        im = ctx.imager(theta, lam, (u, v, w), ("simple",))
        sky = torch.zeros((im.N, im.N), dtype=torch.float64, device=dev)
        sky[im.N // 3, im.N // 2], sky[im.N // 2, im.N // 3] = 1.0, 0.7
        vis = im.predict(sky) + torch.randn(nvis, dtype=torch.float64, device=dev, generator=g).to(torch.complex128)
        model, out = torch.zeros_like(sky), torch.zeros_like(sky)
        kw = dict(model=model, out=out, gain=0.1, niter=niter, patch=256)
        for name, extra in (("deconvolve", {}), ("deconvolve_auto", dict(nsigma=3.0))):
            r = replayed(torch, lambda: im.deconvolve(vis, nmajor, **kw, **extra), model.zero_, reps)
            rows.append(dict(base, what="loop", form=name, N=im.N, nvis=nvis, nmajor=nmajor, niter=niter, patch=256, **r))
        rows[-1]["noise_step_us_per_major_cycle"] = (rows[-1]["median_ms"] - rows[-2]["median_ms"]) * 1e3 / nmajor
        im.close()
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_n2400.jsonl"))
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
    return 0 if len({r["what"] for r in rows}) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
