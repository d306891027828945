#!/usr/bin/env python3
"""Joint CLEAN at N = 2400 (the driver's image size), gain 0.1, niter = 300, for patch 0 (the whole PSF) and 128:
  jclean   ctx.jclean on device tensors for (P, Q) = (1, 1), (4, 1), (4, 4), (8, 8) - one plane, four Stokes planes with
           one PSF, four and eight channels with their own PSFs; the sum for one PSF per plane, the sum of squares for the
           shared one - microseconds per iteration, enqueued eagerly (2 + 2 * niter launches from the host) and replayed
           from a captured graph; next to each the traffic floor, (2P + Q) * 8 B per cell of the updated region at
           6.29 TB/s;
  4xclean  the P = 4, Q = 1 images as four successive ctx.clean calls of niter iterations each, the same way: what a user
           without the joint form runs (and what puts the four component lists at four sets of cells).
Nothing is gated on these times.  Every step is a process of its own under `timeout`, and the steps are chained: a step
that fails, faults or runs out of time ends the run, and nothing more is started on the device.
usage: python tools/jclean_timing.py [--reps 5] [--out profiles/jclean_timing.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mfclean_timing import graphed, timed  # noqa: E402

N, NITER, GAIN, COPY_RATE = 2400, 300, 0.1, 6.29e12
STEPS = [("jclean", P, Q, patch, 240) for P, Q in ((1, 1), (4, 1), (4, 4), (8, 8)) for patch in (0, 128)] + \
        [("4xclean", 4, 1, patch, 240) for patch in (0, 128)]


def inputs(torch, dev, P, Q):
    """Q PSFs from random, point-symmetric uv coverages, normalised to 1 at (N / 2, N / 2); 25 point sources at shared
    positions with per-plane amplitudes - signed for a shared PSF - convolved with each plane's PSF (circularly: this is a
    timing input), noise of 1e-3"""
    g = torch.Generator(device=dev).manual_seed(2400)
    c = N // 2
    ax = (torch.arange(N, device=dev, dtype=torch.float64) - c) / c
    taper = torch.exp(-2.0 * (ax[:, None] ** 2 + ax[None, :] ** 2))
    idx = (2 * c - torch.arange(N, device=dev)) % N
    psfs = []
    for q in range(Q):
        w = (torch.rand((N, N), dtype=torch.float64, device=dev, generator=g) < 0.04 * taper).to(torch.float64)
        w = w + w[idx][:, idx]
        psf = torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(w))).real
        psfs.append(psf / psf[c, c])
    psfs = torch.stack(psfs).contiguous()
    pos = torch.randint(N // 4, N - N // 4, (25, 2), device=dev, generator=g)
    amp = torch.rand((P, 25), dtype=torch.float64, device=dev, generator=g) * 0.8 + 0.2
    if Q == 1:
        amp = amp * (torch.randint(0, 2, (P, 25), device=dev, generator=g).to(torch.float64) * 2.0 - 1.0)
    img = []
    for p in range(P):
        sky = torch.zeros((N, N), dtype=torch.float64, device=dev)
        sky[pos[:, 0], pos[:, 1]] = amp[p]
        img.append(torch.fft.ifft2(torch.fft.fft2(sky) * torch.fft.fft2(torch.fft.ifftshift(psfs[p if Q == P else 0]))).real)
    img = torch.stack(img) + 1e-3 * torch.randn((P, N, N), dtype=torch.float64, device=dev, generator=g)
    return psfs, img.contiguous()


def step(what, P, Q, patch, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    psfs, img = inputs(torch, dev, P, Q)
    res, models = img.clone(), torch.zeros_like(img)

    def reset():
        res.copy_(img)
        models.zero_()

    ctx = gridhip.Context(0)
    kw = dict(gain=GAIN, niter=NITER, patch=patch, threshold=0.0)
    metric = "sumsq" if Q == 1 and P > 1 else "sum"
    if what == "jclean":
        call = lambda: ctx.jclean(res, psfs, metric, models=models, **kw)  # noqa: E731
        iterations, bytes_per_cell = NITER, 8.0 * (2 * P + Q)
    else:
        call = lambda: [ctx.clean(res[p], psfs[0], model=models[p], **kw) for p in range(P)][-1]  # noqa: E731
        iterations, bytes_per_cell = P * NITER, 24.0
    eager = timed(torch, call, reset, reps)
    graph, (_, _, stats) = graphed(torch, call)
    replay = timed(torch, graph.replay, reset, reps)
    side = min(2 * patch + 1, N) if patch else N
    row = {"what": what, "P": P, "Q": Q, "metric": metric if what == "jclean" else None, "N": N, "niter": NITER, "gain": GAIN,
           "patch": patch, "device": torch.cuda.get_device_name(0), "eager": eager, "graph": replay,
           "iterations": stats.cpu().tolist()[0], "total_iterations": iterations,
           "us_per_iteration_eager": eager["median_ms"] * 1e3 / iterations,
           "us_per_iteration_graph": replay["median_ms"] * 1e3 / iterations,
           "floor_us": bytes_per_cell * side * side / COPY_RATE * 1e6,
           "floor_is": f"{bytes_per_cell:.0f} B x the region's cells (whole PSF: the peak at the centre) at 6.29 TB/s"}
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jclean_timing.jsonl"))
    ap.add_argument("--step", nargs=4, metavar=("WHAT", "P", "Q", "PATCH"), help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        print("ROW " + json.dumps(step(args.step[0], *(int(v) for v in args.step[1:]), args.reps)), flush=True)
        return 0
    rows = []
    for what, P, Q, patch, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", what, str(P), str(Q), str(patch)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} P {P} Q {Q} patch {patch} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    # the comparator: the four planes' joint clean against four cleans, per call of niter (joint) and 4 * niter (plain)
    # iterations, and per iteration of either
    joint = {r["patch"]: r for r in rows if r["what"] == "jclean" and (r["P"], r["Q"]) == (4, 1)}
    hogbom = {r["patch"]: r for r in rows if r["what"] == "jclean" and r["P"] == 1}
    for r in rows:
        if r["what"] == "4xclean":
            j = joint[r["patch"]]
            r["joint_call_over_four_cleans_graph"] = j["graph"]["median_ms"] / r["graph"]["median_ms"]
            r["joint_call_over_four_cleans_eager"] = j["eager"]["median_ms"] / r["eager"]["median_ms"]
        else:
            r["over_one_plane_graph"] = r["us_per_iteration_graph"] / hogbom[r["patch"]]["us_per_iteration_graph"]
            r["traffic_model"] = (2 * r["P"] + r["Q"]) / 3.0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
