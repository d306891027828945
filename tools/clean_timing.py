#!/usr/bin/env python3
"""Hogbom CLEAN at N = 2400 (the driver's image size), niter = 1000, gain 0.1, for patch 0 (the whole PSF) and 256:
  native   ctx.clean on device tensors: microseconds per iteration, enqueued eagerly (2 + 2 * niter launches from the
           host) and replayed from a captured graph (what a captured major-cycle loop pays);
  torch    the same loop written in torch on the same device and inputs - abs, argmax, .item(), a sliced subtraction -
           which is what a user has to write without the library (the parent commit has no counterpart to time);
  stopped  the time of a launch after the stop flag is set: a call whose threshold stops it at once, 2000 launches that
           return at their first instruction, against the same call with niter = 0.
Next to each native figure: the traffic floor, 24 B per cell of the updated region at 6.29 TB/s.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/clean_timing.py [--reps 5] [--out profiles/clean_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

N, NITER, GAIN, COPY_RATE = 2400, 1000, 0.1, 6.29e12
STEPS = [("native", 0, 240), ("native", 256, 240), ("torch", 0, 300), ("torch", 256, 300), ("stopped", 0, 240)]


def inputs(torch, dev):
    """a PSF from a random, point-symmetric uv coverage through the centred inverse transform, normalised to 1 at
    (N / 2, N / 2); 25 point sources of both signs in the inner half convolved with it (circularly: this is a timing
    input), noise of 1e-3"""
    g = torch.Generator(device=dev).manual_seed(2400)
    c = N // 2
    ax = (torch.arange(N, device=dev, dtype=torch.float64) - c) / c
    taper = torch.exp(-2.0 * (ax[:, None] ** 2 + ax[None, :] ** 2))
    w = (torch.rand((N, N), dtype=torch.float64, device=dev, generator=g) < 0.04 * taper).to(torch.float64)
    idx = (2 * c - torch.arange(N, device=dev)) % N
    w = w + w[idx][:, idx]
    psf = torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(w))).real
    psf = (psf / psf[c, c]).contiguous()
    sky = torch.zeros((N, N), dtype=torch.float64, device=dev)
    pos = torch.randint(N // 4, N - N // 4, (25, 2), device=dev, generator=g)
    amp = (torch.rand(25, dtype=torch.float64, device=dev, generator=g) * 0.8 + 0.2) * \
        (torch.randint(0, 2, (25,), device=dev, generator=g) * 2 - 1)
    sky[pos[:, 0], pos[:, 1]] = amp
    img = torch.fft.ifft2(torch.fft.fft2(sky) * torch.fft.fft2(torch.fft.ifftshift(psf))).real
    img = img + 1e-3 * torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    return psf, img.contiguous()


def torch_clean(torch, res, psf, model, patch):
    c = N // 2
    for _ in range(NITER):
        k = int(torch.argmax(res.abs()).item())
        y, x = divmod(k, N)
        f = GAIN * res[y, x]
        model[y, x] += f
        ylo, yhi, xlo, xhi = max(0, y - c), min(N - 1, y - c + N - 1), max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        res[ylo:yhi + 1, xlo:xhi + 1] -= f * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]


def timed(torch, fn, reset, reps):
    """device milliseconds of fn() between two events, `reps` times after one warm-up, reset() before each"""
    ms = []
    for rep in range(reps + 1):
        reset()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def step(what, patch, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    psf, img = inputs(torch, dev)
    res, model = img.clone(), torch.zeros_like(img)

    def reset():
        res.copy_(img)
        model.zero_()

    row = {"what": what, "N": N, "niter": NITER, "gain": GAIN, "patch": patch, "device": torch.cuda.get_device_name(0)}
    if what == "torch":
        r = timed(torch, lambda: torch_clean(torch, res, psf, model, patch), reset, reps)
        row.update(r, us_per_iteration=r["median_ms"] * 1e3 / NITER)
        return row
    ctx = gridhip.Context(0)
    kw = dict(gain=GAIN, niter=NITER, patch=patch, model=model, threshold=1e30 if what == "stopped" else 0.0)

    def graphed(**kw):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            ctx.clean(res, psf, **kw)  # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = ctx.clean(res, psf, **kw)
        torch.cuda.synchronize()
        return graph, out

    eager = timed(torch, lambda: ctx.clean(res, psf, **kw), reset, reps)
    graph, (_, _, stats) = graphed(**kw)
    replay = timed(torch, graph.replay, reset, reps)
    done = stats.cpu().tolist()
    if what == "native":
        side = min(2 * patch + 1, N) if patch else N
        native = (model.clone(), res.clone())
        reset()
        torch_clean(torch, res, psf, model, patch)
        peak = img.abs().max()
        row.update(eager=eager, graph=replay, iterations=done[0], us_per_iteration_eager=eager["median_ms"] * 1e3 / NITER,
                   us_per_iteration_graph=replay["median_ms"] * 1e3 / NITER,
                   floor_us=24.0 * side * side / COPY_RATE * 1e6, floor_is="24 B x the region's cells (whole PSF: the "
                   "peak at the centre) at 6.29 TB/s",
                   rel_diff_vs_torch_loop=max(((native[0] - model).abs().max() / peak).item(),
                                              ((native[1] - res).abs().max() / peak).item()))
    else:
        kw0 = dict(kw, niter=0)
        eager0 = timed(torch, lambda: ctx.clean(res, psf, **kw0), reset, reps)
        graph0, _ = graphed(**kw0)
        replay0 = timed(torch, graph0.replay, reset, reps)
        row.update(eager=eager, graph=replay, eager_niter0=eager0, graph_niter0=replay0, iterations=done[0],
                   launches_stopped=2 * NITER,
                   us_per_stopped_launch_eager=(eager["median_ms"] - eager0["median_ms"]) * 1e3 / (2 * NITER),
                   us_per_stopped_launch_graph=(replay["median_ms"] - replay0["median_ms"]) * 1e3 / (2 * NITER))
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_n2400.jsonl"))
    ap.add_argument("--step", nargs=2, metavar=("WHAT", "PATCH"), help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        print("ROW " + json.dumps(step(args.step[0], int(args.step[1]), args.reps)), flush=True)
        return 0
    rows = []
    for what, patch, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", what, str(patch)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} patch {patch} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    native = {r["patch"]: r for r in rows if r["what"] == "native"}
    for r in rows:
        if r["what"] == "torch":
            r["torch_over_native_graph"] = r["us_per_iteration"] / native[r["patch"]]["us_per_iteration_graph"]
            r["torch_over_native_eager"] = r["us_per_iteration"] / native[r["patch"]]["us_per_iteration_eager"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
