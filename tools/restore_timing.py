#!/usr/bin/env python3
"""The restoring beam and the restore at N = 2400 (the driver's image size) and 4096, for supports 8, 16 and 32 and a
model of 0, 100 and 10 000 components (uniformly scattered; a CLEAN model is of this kind):
  fit      ctx.fit_beam on a device PSF: microseconds per call, window 8 and 32;
  native   ctx.restore on device tensors with an explicit support: milliseconds per call, replayed from a captured graph
           of back-to-back calls (as is the fit);
  torch    the same restore written in torch on the same device and inputs, as an fp64 FFT convolution - rfft2 of the
           model, times the (precomputed) transform of the sampled beam, irfft2, plus the residual - which is what a
           user writes without the library.  Its result differs from the direct sum by the wrap-around at the edges and
           the beam beyond `support`; the largest difference is recorded, not asserted.
Next to each native figure: the traffic floor, 3 x 8 B x N^2 at 6.29 TB/s (the copy rate the other tools use), the
arithmetic floor, (2 support + 1)^2 multiply-adds per cell at 39.3 T multiply-adds per second (78.6 TFLOP/s fp64
vector), and the time as a fraction of the larger; for the empty model the tap loop is skipped everywhere, so its
floor is the traffic alone.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/restore_timing.py [--reps 20] [--out profiles/restore_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

COPY_RATE, FMA_RATE = 6.29e12, 39.3e12
SIZES, SUPPORTS, COMPONENTS = (2400, 4096), (8, 16, 32), (0, 100, 10000)
# lambda_min R^2 = ln 1e9 at R = support: the beam each support is sized for (Context.restore's rule), axis ratio 0.7
BEAM = {s: [20.72 / (s * s), 0.0, 20.72 / (0.49 * s * s), 0, 0, 0, 8.0, 1.0] for s in SUPPORTS}


def timed(torch, fn, reps, graph=False):
    """device milliseconds per fn() between two events around `inner` calls, `reps` times after a warm-up; inner is
    sized so that a window lasts about 20 ms.  graph: the inner calls are captured once and replayed, so that the
    host's enqueue rate (tens of microseconds per call from Python) is not what is measured."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    inner = max(1, min(200, int(20.0 / max(a.elapsed_time(b), 1e-3))))

    def window():
        for _ in range(inner):
            fn()
    run = window
    if graph:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn()  # warm-up on the capture stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            window()
        torch.cuda.synchronize()
        run = g.replay
        run()
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms), "inner": inner,
            "graph": graph}


def step(N, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    ctx = gridhip.Context(0)
    rows = []
    base = {"N": N, "device": torch.cuda.get_device_name(0)}
    # the fit: a Gaussian PSF of 5 x 7 cells FWHM with a ripple
    c = N // 2
    ax = torch.arange(N, device=dev, dtype=torch.float64) - c
    psf = torch.exp(-(0.11 * ax[None, :] ** 2 + 0.057 * ax[:, None] ** 2)) * \
        (1.0 + 0.01 * torch.cos(0.3 * ax[None, :]) * torch.cos(0.2 * ax[:, None]))
    psf = psf.contiguous()
    for window in (8, 32):
        r = timed(torch, lambda: ctx.fit_beam(psf, window, 0.5), reps, graph=True)
        beam = ctx.fit_beam(psf, window, 0.5).cpu().tolist()
        rows.append(dict(base, what="fit", window=window, us_per_call=r["median_ms"] * 1e3, ncells=beam[6], ok=beam[7],
                         bmaj=beam[3], bmin=beam[4], **r))
    res = 1e-3 * torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty_like(res)
    floor_traffic = 24.0 * N * N / COPY_RATE * 1e3
    for ncomp in COMPONENTS:
        model = torch.zeros((N, N), dtype=torch.float64, device=dev)
        if ncomp:
            pos = torch.randint(0, N, (ncomp, 2), device=dev, generator=g)
            model[pos[:, 0], pos[:, 1]] = torch.rand(ncomp, dtype=torch.float64, device=dev, generator=g) + 0.1
        for s in SUPPORTS:
            beam = torch.tensor(BEAM[s], dtype=torch.float64, device=dev)
            nat = timed(torch, lambda: ctx.restore(model, res, beam, s, out=out), reps, graph=True)
            native = out.clone()
            # tiles of 32 x 64 cells whose window (the tile and its halo) holds a component: the ones that run the taps
            occ = torch.nn.functional.max_pool2d((model != 0)[None, None].to(torch.float32), 2 * s + 1, 1, s)[0, 0]
            busy = torch.nn.functional.max_pool2d(occ[None, None], (32, 64), (32, 64), ceil_mode=True).sum().item()
            tiles = ((N + 31) // 32) * ((N + 63) // 64)
            floor_fma = busy * 32 * 64 * (2 * s + 1) ** 2 / FMA_RATE * 1e3
            A, B, Cq = BEAM[s][:3]
            d = torch.fft.fftfreq(N, 1.0 / N).to(dev).to(torch.float64)  # 0, 1, ..., -1: the beam wrapped about cell 0
            kern = torch.exp(-(A * d[None, :] ** 2 + 2 * B * d[None, :] * d[:, None] + Cq * d[:, None] ** 2))
            kf = torch.fft.rfft2(kern)
            tor = timed(torch, lambda: torch.add(torch.fft.irfft2(torch.fft.rfft2(model) * kf, s=(N, N)), res, out=out), reps)
            diff = (out - native).abs().max().item()
            floor = max(floor_traffic, floor_fma)
            rows.append(dict(base, what="restore", support=s, components=ncomp, tiles=tiles, tiles_with_taps=int(busy),
                             native=nat, torch_fft=tor, native_ms=nat["median_ms"], torch_fft_ms=tor["median_ms"],
                             torch_over_native=tor["median_ms"] / nat["median_ms"], floor_traffic_ms=floor_traffic,
                             floor_fma_ms=floor_fma, bound_by="traffic" if floor_traffic >= floor_fma else "fp64 rate",
                             fraction_of_floor=floor / nat["median_ms"], max_abs_diff_vs_fft=diff))
    # a dense model: every tile runs its taps
    model = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    for s in SUPPORTS:
        beam = torch.tensor(BEAM[s], dtype=torch.float64, device=dev)
        nat = timed(torch, lambda: ctx.restore(model, res, beam, s, out=out), reps, graph=True)
        floor_fma = N * N * (2 * s + 1) ** 2 / FMA_RATE * 1e3
        A, B, Cq = BEAM[s][:3]
        d = torch.fft.fftfreq(N, 1.0 / N).to(dev).to(torch.float64)
        kf = torch.fft.rfft2(torch.exp(-(A * d[None, :] ** 2 + 2 * B * d[None, :] * d[:, None] + Cq * d[:, None] ** 2)))
        tor = timed(torch, lambda: torch.add(torch.fft.irfft2(torch.fft.rfft2(model) * kf, s=(N, N)), res, out=out), reps)
        floor = max(floor_traffic, floor_fma)
        rows.append(dict(base, what="restore", support=s, components="dense", native=nat, torch_fft=tor,
                         native_ms=nat["median_ms"], torch_fft_ms=tor["median_ms"],
                         torch_over_native=tor["median_ms"] / nat["median_ms"], floor_traffic_ms=floor_traffic,
                         floor_fma_ms=floor_fma, bound_by="traffic" if floor_traffic >= floor_fma else "fp64 rate",
                         fraction_of_floor=floor / nat["median_ms"]))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_n2400.jsonl"))
    ap.add_argument("--step", metavar="N", help="run one size in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in step(int(args.step), args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for N in SIZES:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", str(N)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step N {N} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        for line in got:
            rows.append(json.loads(line))
            print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
