#!/usr/bin/env python3
"""Auto-masking at N = 2400 (the driver's image size):
  images   gridhip_automask_dev (nsigma 5 / 2.5 of the image's own sigma, min_cells 4, grow 2) and gridhip_image_stats_dev
           on three images - noise only, noise plus 300 Gaussian islands, and one all-set component (a constant above
           fixed levels) - eagerly and replayed from a captured graph, with their ratio;
  loop     one Imager.deconvolve call with nsigma / peak_frac (gridhip_imager_deconvolve_auto_dev) and one with
           automask={...} (gridhip_imager_deconvolve_automask_dev) on the same simple imager of 2e6 visibilities, the
           same nmajor and niter: what the mask update costs a major cycle.
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/automask_timing.py [--reps 5] [--out profiles/automask_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

N, NMAJOR, NITER, NVIS = 2400, 3, 200, 2_000_000
STEPS = [("images", 300), ("loop", 300)]
AM = dict(nsigma=(5, 2.5), min_cells=4, grow=2)


def images(torch, dev):
    g = torch.Generator(device=dev).manual_seed(2400)
    noise = 1e-3 * torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    ax = torch.arange(N, device=dev, dtype=torch.float64)
    isl = noise.clone()
    pos = torch.randint(20, N - 20, (300, 2), device=dev, generator=g)
    amp = torch.rand(300, dtype=torch.float64, device=dev, generator=g) * 0.1 + 0.01
    wid = torch.rand(300, dtype=torch.float64, device=dev, generator=g) * 3.0 + 1.0
    for (y, x), a, w in zip(pos.tolist(), amp.tolist(), wid.tolist()):
        ys, xs = slice(max(0, y - 20), y + 21), slice(max(0, x - 20), x + 21)
        isl[ys, xs] += a * torch.exp(-0.5 * ((ax[ys, None] - y) ** 2 + (ax[None, xs] - x) ** 2) / w ** 2)
    return {"noise": noise, "islands": isl, "all_set": torch.ones((N, N), dtype=torch.float64, device=dev)}


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


def graphed(torch, fn):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = fn()
    torch.cuda.synchronize()
    return graph, out


def step_images(reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    rows = []
    mask = torch.zeros((N, N), dtype=torch.uint8, device=dev)
    for name, img in images(torch, dev).items():
        ist = ctx.image_stats(img)
        kw = dict(AM, noise=ist[3:4]) if name != "all_set" else dict(AM, nsigma=0, thr=(0.5, 0.25))
        row = {"what": "automask", "image": name, "N": N, "device": torch.cuda.get_device_name(0),
               "options": {k: v for k, v in kw.items() if k != "noise"}}
        row["automask_eager"] = timed(torch, lambda: ctx.automask(img, mask, **kw), mask.zero_, reps)
        graph, (_, st) = graphed(torch, lambda: ctx.automask(img, mask, **kw))
        row["automask_graph"] = timed(torch, graph.replay, mask.zero_, reps)
        row["stats"] = st.cpu().tolist()
        row["image_stats_eager"] = timed(torch, lambda: ctx.image_stats(img), lambda: None, reps)
        graph, _ = graphed(torch, lambda: ctx.image_stats(img))
        row["image_stats_graph"] = timed(torch, graph.replay, lambda: None, reps)
        row["automask_over_image_stats_graph"] = row["automask_graph"]["median_ms"] / row["image_stats_graph"]["median_ms"]
        rows.append(row)
    ctx.close()
    return rows


def step_loop(reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    theta, lam = 0.08, 30000  # image_size = 2400
    g = torch.Generator(device=dev).manual_seed(7)
    u, v = ((torch.rand(NVIS, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.8 * lam for _ in range(2))
    w = torch.zeros(NVIS, dtype=torch.float64, device=dev)
    im = ctx.imager(theta, lam, (u, v, w), ("simple",))
    assert im.N == N
    sky = torch.zeros((N, N), dtype=torch.float64, device=dev)
    pos = torch.randint(N // 4, N - N // 4, (25, 2), device=dev, generator=g)
    sky[pos[:, 0], pos[:, 1]] = torch.rand(25, dtype=torch.float64, device=dev, generator=g) * 0.8 + 0.2
    vis = im.predict(sky) + 0.5 * torch.randn(NVIS, dtype=torch.complex128, device=dev, generator=g)
    model, out = torch.zeros((N, N), dtype=torch.float64, device=dev), torch.zeros((N, N), dtype=torch.float64, device=dev)
    mask = torch.zeros((N, N), dtype=torch.uint8, device=dev)
    kw = dict(model=model, out=out, gain=0.1, niter=NITER, nsigma=3.0, peak_frac=0.05)

    def reset():
        model.zero_()
        mask.zero_()
    row = {"what": "loop", "N": N, "nvis": NVIS, "nmajor": NMAJOR, "niter": NITER, "kind": "simple",
           "device": torch.cuda.get_device_name(0), "automask": {k: v for k, v in AM.items()}}
    row["cycle"] = timed(torch, lambda: im.cycle(vis, model, out), reset, reps)
    row["deconvolve_auto"] = timed(torch, lambda: im.deconvolve(vis, NMAJOR, **kw), reset, reps)
    r = im.deconvolve(vis, NMAJOR, **kw)
    row["deconvolve_auto_iterations"] = r[2][:, 0].cpu().tolist()
    row["deconvolve_automask"] = timed(torch, lambda: im.deconvolve(vis, NMAJOR, mask=mask, automask=AM, **kw), reset, reps)
    reset()
    r = im.deconvolve(vis, NMAJOR, mask=mask, automask=AM, **kw)
    row["deconvolve_automask_iterations"] = r[2][:, 0].cpu().tolist()
    row["astats"] = r[5].cpu().tolist()
    row["extra_ms_per_major_cycle"] = (row["deconvolve_automask"]["median_ms"] - row["deconvolve_auto"]["median_ms"]) / NMAJOR
    im.close()
    ctx.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "automask_n2400.jsonl"))
    ap.add_argument("--step", help="run one step in this process (internal)")
    args = ap.parse_args()
    if args.step:
        for row in (step_images if args.step == "images" else step_loop)(args.reps):
            print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = []
    for what, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps",
                            str(args.reps), "--step", what], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {what} ended with status {r.returncode}: nothing more is started", flush=True)
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
