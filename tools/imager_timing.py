#!/usr/bin/env python3
"""One major cycle at N = 2400 and 10^6 visibilities, for every kind (simple, conv, w_cache, aw), on the same box in the
same run:
  (a) predict_dev (residual form) + do_imaging[_aw]_dev, the two calls a cycle is without an imager;
  (b) imager.cycle(vis, model), the same image from an imager;
  (c) the imager's creation (host clock around a synchronised call: it allocates and synchronises).
(a) and (b) alternate, rep by rep, each between two device events; the median of --reps timed pairs after warm-up calls,
with min and max as the spread.  The stream and tables are tools/predict_timing.py's.  "clock_khz" / "aw_clock_khz": the
shader clock the last tile kernel / aw kernel builder held, where the library could read it.
usage: python tools/imager_timing.py [--reps 20] [--warmup 3] [--out profiles/imager_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
import torch  # noqa: E402

import bench  # noqa: E402
import gridhip  # noqa: E402

THETA, LAM, N, n = 0.08, 30000, 2400, 1_000_000
KO = {"wstep": 2000, "qpx": 4, "npixFF": 256, "npixKern": 15}
W, Q, S, A = 128, 8, 15, 512


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def alternate(fa, fb, reps, warmup):
    """device milliseconds per call of fa() and fb(), taken alternately"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record()
        fa()
        e[1].record()
        fb()
        e[2].record()
    torch.cuda.synchronize()
    return stats([e[0].elapsed_time(e[1]) for e in ev]), stats([e[1].elapsed_time(e[2]) for e in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imager_n2400.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0x9E3779B9)
    uni = lambda lo, hi: torch.rand(n, dtype=torch.float64, device=dev, generator=g) * (hi - lo) + lo
    u, v = uni(-0.45, 0.45) * LAM, uni(-0.45, 0.45) * LAM
    w = uni(-0.5, 0.5) * 20 * KO["wstep"]
    vis = torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=g),
                        torch.randn(n, dtype=torch.float64, device=dev, generator=g))
    model = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    kv = bench.synth_kernels(1, 8, 7, dev)[0]
    au, av, awb, a1, a2, avis = bench.synth_aw_stream(n, N, W, S, A, 0x5EEDC0DE, dev)
    wvals = (torch.arange(W, dtype=torch.float64, device=dev) - W // 2) * 100.0
    awk, aak = bench.synth_kernels(W, Q, S, dev), bench.synth_akernels(A, S, dev)
    auvw = (au * LAM, av * LAM, wvals[awb])
    ctx = gridhip.Context(0)
    assert ctx.image_size(THETA, LAM) == N
    head = {"N": N, "n": n, "device": torch.cuda.get_device_name(0)}
    rows = []

    def rec(what, r, **extra):
        row = dict(head, what=what, **r, **extra)
        rows.append(row)
        print(json.dumps(row), flush=True)

    kinds = {
        "simple": ((u, v, w), ("simple",), None, None, vis),
        "conv (Q 8, 7x7)": ((u, v, w), ("conv", kv), None, None, vis),
        "w_cache (wstep 2000, qpx 4, npixFF 256, 15x15)": ((u, v, w), ("w_cache", KO), None, None, vis),
        "aw (15x15, Q 8, 128 planes, 512 antennas)": (auvw, ("aw", awk, wvals, aak), a1, a2, avis),
    }
    res = torch.empty(n, dtype=torch.complex128, device=dev)
    img = torch.empty((N, N), dtype=torch.float64, device=dev)
    for name, (uvw, imgfn, b1, b2, vs) in kinds.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        im = ctx.imager(THETA, LAM, uvw, imgfn, a1=b1, a2=b2)
        torch.cuda.synchronize()
        create_ms = (time.perf_counter() - t0) * 1e3
        ims = []
        for _ in range(2):  # (a second creation: scratch and code objects are warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            im2 = ctx.imager(THETA, LAM, uvw, imgfn, a1=b1, a2=b2)
            torch.cuda.synchronize()
            ims.append((time.perf_counter() - t0) * 1e3)
            im2.close()

        def two_calls():
            ctx.predict(THETA, LAM, uvw, model, imgfn, a1=b1, a2=b2, vis_sub=vs, out=res)
            return ctx.do_imaging(THETA, LAM, uvw, b1, b2, None, None, res, imgfn)[0]

        cycle = lambda: im.cycle(vs, model, out=img)
        ref = two_calls()
        cycle()
        torch.cuda.synchronize()
        err = ((img - ref).abs().max() / ref.abs().max()).item()
        a, b = alternate(two_calls, cycle, args.reps, args.warmup)
        clock = {k: ctx.get_option(k) for k in ("clock_khz", "aw_clock_khz")}
        rec(f"(a) predict_dev + do_imaging{'_aw' if imgfn[0] == 'aw' else ''}_dev {name}", a, **clock)
        rec(f"(b) imager.cycle {name}", b, a_over_b=a["median_ms"] / b["median_ms"],
            a_minus_b_ms=a["median_ms"] - b["median_ms"], b_max_below_a_min=b["max_ms"] < a["min_ms"],
            rel_err_vs_two_calls=err, **clock)
        rec(f"(c) imager creation {name}", {"first_ms": create_ms, "warm_ms": min(ims)})
        im.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
