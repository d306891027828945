#!/usr/bin/env python3
"""A major cycle on layered grids three ways, on the GPU and under no profiler.
  The stream: n visibilities, u, v uniform in +-0.4 lam, w uniform in +-2000, theta = 0.1, lam = 20480 (N = 2048),
  wstep = 100, S = 15, M = 8 planes per layer (6 layers on either stream), a random model.  One cycle is
  image = do_imaging(vis - predict(model)) with uniform weights.
  (a) by hand  two Context.wstack handles - one on the stream as given, one on the mirrored stream - and per cycle
               predict(model, vis_sub=vis) of the first, one torch pass (conjugate where mirrored, times the weight), image of
               the second, one torch pass (times 2 / pmax).  Only calls that exist without the imager kind: on a checkout
               without it the tool times (a) alone and says so.
  (b) Imager.cycle of ctx.imager(..., ("wstack", ko)) with the context option wstack_middle = 1
  (c) the same with wstack_middle = 0 (the default)
  The three are timed in turns - a, b, c, a, b, c, ... - in one process, so that a drift of the clock or of the memory's
  state falls on all of them alike.  Events on the stream around eager calls, a warm-up first, the median and the extremes of
  `reps` runs; the spread of (a) is the yardstick's own noise.  Then Imager.deconvolve(nmajor=2, niter=100) of the kind.
Every n is a process of its own under `timeout`, and the steps are chained: one that fails, faults or runs out of time ends
the run.
usage: python tools/wstack_imager_timing.py [--reps 5] [--out profiles/wstack_imager_timing.jsonl]  (--out is appended to)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))

THETA, LAM, WSTEP, WMAX, QPX, NPIXFF, S, M = 0.1, 20480, 100, 2000.0, 4, 64, 15, 8
SIZES = [4_000_000, 32_000_000]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed_in_turns(torch, fns, reps):
    """{name: summary} of the callables, run in turns after one warm-up each"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: summary(v) for k, v in ms.items()}


def step(n, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    N = ctx.image_size(THETA, LAM)
    gen = torch.Generator(device=dev).manual_seed(5)
    r = lambda lo, hi: torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo  # noqa: E731
    u, v, w = r(-0.4 * LAM, 0.4 * LAM), r(-0.4 * LAM, 0.4 * LAM), r(-WMAX, WMAX)
    vis = torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=gen),
                        torch.randn(n, dtype=torch.float64, device=dev, generator=gen))
    model = torch.randn((N, N), dtype=torch.float64, device=dev, generator=gen)
    ko = dict(wstep=WSTEP, planes=M, qpx=QPX, npixFF=NPIXFF, npixKern=S)
    row = {"step": "cycle", "N": N, "n": n, "theta": THETA, "wstep": WSTEP, "wmax": WMAX, "qpx": QPX, "npixFF": NPIXFF, "S": S,
           "planes": M, "device": torch.cuda.get_device_name(0)}

    # (a) by hand
    sign = torch.where(v < 0, -1.0, 1.0).to(torch.float64)
    mu, mv, mw = u * sign, v * sign, w * sign
    wt, _ = ctx.weights(THETA, LAM, (mu, mv), "uniform")
    ws_u, ws_m = ctx.wstack(THETA, LAM, (u, v, w), ko), ctx.wstack(THETA, LAM, (mu, mv, mw), ko)
    row.update(layers=[ws_u.layers, ws_m.layers], occupied=[ws_u.occupied, ws_m.occupied])
    sw2 = torch.stack([wt, wt * sign], dim=1).contiguous()  # re and im of the weighted, mirrored residual in one product
    del mu, mv, mw
    res, x = torch.empty_like(vis), torch.empty_like(vis)
    img_a = torch.empty((N, N), dtype=torch.float64, device=dev)
    scale = 1.0 / ws_m.image(wt.to(torch.complex128)).max()  # 2 / pmax, pmax = max(2 Re D(wt)); a device scalar

    def by_hand():
        ws_u.predict(model, vis_sub=vis, out=res)
        torch.mul(torch.view_as_real(res), sw2, out=torch.view_as_real(x))
        ws_m.image(x, out=img_a)
        img_a.mul_(scale)

    fns = {"by_hand": by_hand}
    im = None
    try:
        im = ctx.imager(THETA, LAM, (u, v, w), ("wstack", ko))
    except ValueError as e:  # a checkout without the kind: (a) alone
        row["imager"] = f"not available ({e})"
    if im is not None:
        img_b = torch.empty((N, N), dtype=torch.float64, device=dev)
        res_b = torch.empty_like(vis)

        def cycle(middle):
            ctx.set_option("wstack_middle", middle)
            im.cycle(vis, model, out=img_b, vis_res=res_b)
            ctx.set_option("wstack_middle", 0)

        fns["imager_middle_1"] = lambda: cycle(1)
        fns["imager_middle_0"] = lambda: cycle(0)
    row["cycle"] = timed_in_turns(torch, fns, reps)
    if im is not None:
        by_hand()
        cycle(0)
        torch.cuda.synchronize()
        row["agreement"] = float((img_a - img_b).abs().max() / img_a.abs().max())
        row["vis_res_equal"] = bool(torch.equal(torch.view_as_real(res), torch.view_as_real(res_b)))
        row["cycle_no_vis_res"] = timed_in_turns(torch, {"imager_middle_1": lambda: (ctx.set_option("wstack_middle", 1),
                                                                                    im.cycle(vis, model, out=img_b),
                                                                                    ctx.set_option("wstack_middle", 0)),
                                                         "imager_middle_0": lambda: im.cycle(vis, model, out=img_b)}, reps)
        mdl = torch.zeros((N, N), dtype=torch.float64, device=dev)

        def deconvolve():
            mdl.zero_()
            im.deconvolve(vis, 2, model=mdl, out=img_b, niter=100)

        row["deconvolve_nmajor2_niter100"] = timed_in_turns(torch, {"deconvolve": deconvolve}, reps)["deconvolve"]
        im.close()
    ws_u.close(), ws_m.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wstack_imager_timing.jsonl"))
    ap.add_argument("--step", metavar="n", help="run one size in this process (internal)")
    args = ap.parse_args()
    if args.step:
        print("ROW " + json.dumps(step(int(args.step), args.reps)), flush=True)
        return 0
    rows = []
    for n in SIZES:
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                            "--step", str(n)], stdout=subprocess.PIPE, text=True)
        got = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not got:
            print(f"step {n} ended with status {r.returncode}: nothing more is started", flush=True)
            return 1
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
