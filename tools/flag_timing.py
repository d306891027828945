#!/usr/bin/env python3
"""Residual flagging against image_stats, device events, the median of 20 replays of a captured graph:
  stream    one round (niter = 1) of ctx.flag_residuals over 5.76 x 10^6 visibilities - the element count of an N = 2400
            image - at G = 1, and ctx.image_stats at N = 2400 with 8-bit digits (the same digit width and pass structure)
            and with the default 13-bit ones, in the same process; the ratio flag / image_stats(8 bits), beside the ratio
            of the bytes the two stream (40 + 16 x 12 + 12 + 20 against 16 x 8 per element).  Then the same stream at
            G = 64 and 65 (the last group count of the LDS histogram and the first of the global one) and at G = 130816
            (the baselines of 512 antennas); niter = 0 and niter = 3 at G = 1 for the fixed costs and a stopped round;
  imager    three rounds of Imager.flag on the 10^6-visibility w_cache imager of tools/imager_timing.py, per baseline of
            512 antennas, beside its cycle and beside predict alone (flag = predict + the flagging).
Every step is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out
of time ends the run, and nothing more is started on the device.
usage: python tools/flag_timing.py [--reps 20] [--out profiles/flag_n5760000.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 2400
NVIS = N * N
STEPS = [("stream", 400), ("imager", 400)]


def flag_bytes(niter):
    """bytes per visibility: the front pass (16 + 16 + 8 + 8 in, 12 + 1 out), 16 passes of 12 and a clip pass of 12 per
    round, the final pass (4 + 8 in, 8 out)"""
    return 61 + niter * (16 * 12 + 12) + 20


def step(what, reps):
    import torch
    import gridhip
    from noise_timing import replayed
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    rows = []
    base = {"device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device=dev).manual_seed(3)
    randc = lambda n: torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=g),  # noqa: E731
                                    torch.randn(n, dtype=torch.float64, device=dev, generator=g))
    if what == "stream":
        image = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
        stats = {}
        for bits in (8, 13):
            ctx.set_option("noise_bits", bits)
            passes = 2 * ((64 + bits - 1) // bits)
            r = replayed(torch, lambda: ctx.image_stats(image), lambda: None, reps)
            stats[bits] = r["median_ms"]
            rows.append(dict(base, what="image_stats", N=N, digit_bits=bits, passes=passes, bytes_per_element=8 * passes, **r))
        ctx.set_option("noise_bits", 0)
        model = randc(NVIS)
        vis = model + randc(NVIS)
        vis[::1000] *= 50.0
        wt = torch.rand(NVIS, dtype=torch.float64, device=dev, generator=g) + 0.5
        out = torch.empty_like(wt)
        for G, niter in ((1, 1), (64, 1), (65, 1), (130816, 1), (1, 0), (1, 3)):
            group = None if G == 1 else torch.randint(0, G, (NVIS,), dtype=torch.int64, device=dev, generator=g)
            kw = dict(group=group, G=None if G == 1 else G, weights=wt, nsigma=5.0, niter=niter, out=out)
            res = ctx.flag_residuals(vis, model, **kw)
            r = replayed(torch, lambda: ctx.flag_residuals(vis, model, **kw), lambda: None, reps)
            row = dict(base, what="flag_residuals", n=NVIS, G=G, niter=niter, path="lds" if G <= 64 else "global",
                       launches=3 + 33 * niter if niter else 5, bytes_per_element=flag_bytes(niter),
                       stats=[float(x) for x in res[3].tolist()], **r)
            if niter == 1:
                row["over_image_stats_8bit"] = r["median_ms"] / stats[8]
                row["over_image_stats_13bit"] = r["median_ms"] / stats[13]
                row["byte_ratio_to_image_stats_8bit"] = flag_bytes(1) / 128.0
            rows.append(row)
    else:
        import imager_timing as IT
        n = IT.n
        uni = lambda lo, hi: torch.rand(n, dtype=torch.float64, device=dev, generator=g) * (hi - lo) + lo  # noqa: E731
        u, v = uni(-0.45, 0.45) * IT.LAM, uni(-0.45, 0.45) * IT.LAM
        w = uni(-0.5, 0.5) * 20 * IT.KO["wstep"]
        im = ctx.imager(IT.THETA, IT.LAM, (u, v, w), ("w_cache", IT.KO))
        model = torch.zeros((im.N, im.N), dtype=torch.float64, device=dev)
        model[im.N // 3, im.N // 2], model[im.N // 2, im.N // 3] = 1.0, 0.7
        vis = im.predict(model) + 0.01 * randc(n)
        vis[::500] += 3.0
        a1 = torch.randint(0, 511, (n,), dtype=torch.int64, device=dev, generator=g)
        a2 = a1 + 1 + (torch.rand(n, dtype=torch.float64, device=dev, generator=g) * (511 - a1)).to(torch.int64)
        group, G = gridhip.flag_groups(a1, a2)
        wt = torch.ones(n, dtype=torch.float64, device=dev)
        out, img, pred = torch.empty_like(wt), torch.empty_like(model), torch.empty_like(vis)
        head = dict(base, N=im.N, n=n, kind="w_cache (wstep 2000, qpx 4, npixFF 256, 15x15)")
        r = replayed(torch, lambda: im.cycle(vis, model, out=img), lambda: None, reps)
        rows.append(dict(head, what="imager.cycle", **r))
        r = replayed(torch, lambda: im.predict(model, out=pred), lambda: None, reps)
        rows.append(dict(head, what="imager.predict", **r))
        for GG, grp in ((G, group), (1, None)):
            kw = dict(group=grp, G=None if grp is None else GG, weights=wt, nsigma=5.0, min_count=3, niter=3, out=out)
            res = im.flag(model, vis, **kw)
            r = replayed(torch, lambda: im.flag(model, vis, **kw), lambda: None, reps)
            rows.append(dict(head, what="imager.flag", G=GG, niter=3, stats=[float(x) for x in res[3].tolist()],
                             minus_predict_ms=r["median_ms"] - rows[1]["median_ms"],
                             over_cycle=r["median_ms"] / rows[0]["median_ms"], **r))
        im.close()
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flag_n5760000.jsonl"))
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
    return 0 if len({r["what"] for r in rows}) >= 5 else 1


if __name__ == "__main__":
    sys.exit(main())
