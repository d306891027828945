#!/usr/bin/env python3
"""Wide-band imaging at N = 2400 (the driver's image size), gain 0.1, niter = 300, for patch 0 (the whole PSF) and 128:
  mfclean  ctx.mfclean on device tensors for T = 1, 2, 3 Taylor terms: microseconds per iteration, enqueued eagerly
           (2 + 2 * niter launches from the host) and replayed from a captured graph; next to each the traffic floor,
           (4T - 1) * 8 B per cell of the updated region at 6.29 TB/s;
  clean    ctx.clean on the same image and PSF (term 0), the same way: the traffic model predicts a region pass of
           (4T - 1) / 3 times this one;
  cycle    one Imager.mfs_cycle with T = 2 (two transforms and gathers, two scatters and tails) against two plain
           Imager.cycle calls on a w_cache imager of 120 000 visibilities.
Nothing is gated on these times.  Every step is a process of its own under `timeout`, and the steps are chained: a step
that fails, faults or runs out of time ends the run, and nothing more is started on the device.
usage: python tools/mfclean_timing.py [--reps 5] [--out profiles/mfs_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

N, NITER, GAIN, COPY_RATE = 2400, 300, 0.1, 6.29e12
STEPS = [("clean", 1, 0, 240), ("clean", 1, 128, 240)] + \
        [("mfclean", T, patch, 240) for T in (1, 2, 3) for patch in (0, 128)] + [("cycle", 2, 0, 300)]


def inputs(torch, dev, T):
    """2T - 1 spectral PSFs from a random, point-symmetric uv coverage with a random x in [-0.25, 0.25] per occupied cell,
    normalised to P_0 = 1 at (N / 2, N / 2); per term 25 point sources with slopes convolved with them (circularly: this
    is a timing input), noise of 1e-3"""
    g = torch.Generator(device=dev).manual_seed(2400)
    c = N // 2
    ax = (torch.arange(N, device=dev, dtype=torch.float64) - c) / c
    taper = torch.exp(-2.0 * (ax[:, None] ** 2 + ax[None, :] ** 2))
    occ = (torch.rand((N, N), dtype=torch.float64, device=dev, generator=g) < 0.04 * taper).to(torch.float64)
    x = torch.rand((N, N), dtype=torch.float64, device=dev, generator=g) * 0.5 - 0.25
    idx = (2 * c - torch.arange(N, device=dev)) % N
    psfs = []
    for s in range(2 * T - 1):
        w = occ * x ** s
        w = w + w[idx][:, idx]
        psfs.append(torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(w))).real)
    psfs = (torch.stack(psfs) / psfs[0][c, c]).contiguous()
    pos = torch.randint(N // 4, N - N // 4, (25, 2), device=dev, generator=g)
    amp = (torch.rand(25, dtype=torch.float64, device=dev, generator=g) * 0.8 + 0.2)
    alpha = torch.rand(25, dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.5
    sky0, sky1 = (torch.zeros((N, N), dtype=torch.float64, device=dev) for _ in range(2))
    sky0[pos[:, 0], pos[:, 1]] = amp
    sky1[pos[:, 0], pos[:, 1]] = amp * alpha

    def conv(sky, psf):
        return torch.fft.ifft2(torch.fft.fft2(sky) * torch.fft.fft2(torch.fft.ifftshift(psf))).real

    img = torch.stack([conv(sky0, psfs[t]) + (conv(sky1, psfs[t + 1]) if t + 1 < 2 * T - 1 else 0.0) for t in range(T)])
    img = img + 1e-3 * torch.randn((T, N, N), dtype=torch.float64, device=dev, generator=g)
    return psfs, img.contiguous()


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


def graphed(torch, call):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call()  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = call()
    torch.cuda.synchronize()
    return graph, out


def minor_step(what, T, patch, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    psfs, img = inputs(torch, dev, T)
    if what == "clean":
        psfs, img = psfs[0].contiguous(), img[0].contiguous()
    res, model = img.clone(), torch.zeros_like(img)

    def reset():
        res.copy_(img)
        model.zero_()

    ctx = gridhip.Context(0)
    kw = dict(gain=GAIN, niter=NITER, patch=patch, threshold=0.0)
    call = (lambda: ctx.clean(res, psfs, model=model, **kw)) if what == "clean" else \
        (lambda: ctx.mfclean(res, psfs, models=model, **kw))
    eager = timed(torch, call, reset, reps)
    graph, (_, _, stats) = graphed(torch, call)
    replay = timed(torch, graph.replay, reset, reps)
    side = min(2 * patch + 1, N) if patch else N
    bytes_per_cell = 24.0 if what == "clean" else 8.0 * (4 * T - 1)
    row = {"what": what, "T": T, "N": N, "niter": NITER, "gain": GAIN, "patch": patch,
           "device": torch.cuda.get_device_name(0), "eager": eager, "graph": replay, "iterations": stats.cpu().tolist()[0],
           "us_per_iteration_eager": eager["median_ms"] * 1e3 / NITER,
           "us_per_iteration_graph": replay["median_ms"] * 1e3 / NITER,
           "floor_us": bytes_per_cell * side * side / COPY_RATE * 1e6,
           "floor_is": f"{bytes_per_cell:.0f} B x the region's cells (whole PSF: the peak at the centre) at 6.29 TB/s"}
    ctx.close()
    return row


def cycle_step(T, reps):
    import numpy as np
    import torch
    import gridhip
    theta, lam, n = 0.008, 300_000, 120_000
    rng = np.random.default_rng(77)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    uvw = tuple(dev(a) for a in (rng.uniform(-0.45, 0.45, n) * lam, rng.uniform(-0.45, 0.45, n) * lam,
                                 rng.uniform(-1800.0, 1800.0, n)))
    vis = dev(rng.normal(size=n) + 1j * rng.normal(size=n))
    models = dev(rng.normal(size=(T, N, N)))
    ctx = gridhip.Context(0)
    im = ctx.imager(theta, lam, uvw, ("w_cache", {"wstep": 500, "qpx": 4, "npixFF": 64, "npixKern": 15}))
    assert im.N == N
    im.set_spectral(dev(rng.choice(np.linspace(-0.2, 0.2, 8), n)), T)
    out, single = torch.zeros((T, N, N), dtype=torch.float64, device="cuda:0"), [torch.zeros_like(models[0]) for _ in range(T)]

    def plain():
        for t in range(T):
            im.cycle(vis, models[t], out=single[t])

    wide = timed(torch, lambda: im.mfs_cycle(vis, models, out=out), lambda: None, reps)
    two = timed(torch, plain, lambda: None, reps)
    row = {"what": "cycle", "T": T, "N": N, "n": n, "kind": "w_cache", "device": torch.cuda.get_device_name(0),
           "mfs_cycle": wide, "plain_cycles": two, "plain_cycles_count": T,
           "mfs_cycle_over_plain_cycles": wide["median_ms"] / two["median_ms"]}
    im.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfs_n2400.jsonl"))
    ap.add_argument("--step", nargs=3, metavar=("WHAT", "T", "PATCH"), help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        what, T, patch = args.step[0], int(args.step[1]), int(args.step[2])
        row = cycle_step(T, args.reps) if what == "cycle" else minor_step(what, T, patch, args.reps)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for what, T, patch, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", what, str(T), str(patch)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} T {T} patch {patch} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    hogbom = {r["patch"]: r for r in rows if r["what"] == "clean"}
    for r in rows:
        if r["what"] == "mfclean":
            r["over_clean_graph"] = r["us_per_iteration_graph"] / hogbom[r["patch"]]["us_per_iteration_graph"]
            r["traffic_model"] = (4 * r["T"] - 1) / 3.0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
