#!/usr/bin/env python3
"""Prediction at N = 2400 and 10^6 visibilities: device time per call of predict_dev for every kind (simple, conv,
w_cache, aw) beside do_imaging_dev / do_imaging_aw_dev of the same kind and stream, and the split of a prediction
between the transform (head kernel + FFT: ms_prepass of gridhip_timing) and the gather (+ residual epilogue: ms_kernel).
w_cache: also one major cycle (do_imaging_dev, then predict_dev on the un-mirrored w) per repetition, where the w-kernel
cache may be rebuilt when the mirrored and the un-mirrored w ranges differ.  Device events on torch's stream, warm-up
calls first, the median of --reps timed ones.
usage: python tools/predict_timing.py [--reps 20] [--warmup 3] [--out profiles/predict_n2400.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
import torch  # noqa: E402

import bench  # noqa: E402
import gridhip  # noqa: E402

THETA, LAM, N, n = 0.08, 30000, 2400, 1_000_000
KO = {"wstep": 2000, "qpx": 4, "npixFF": 256, "npixKern": 15}  # profiles/r03_do_imaging_n2400.jsonl's w_cache shape
W, Q, S, A = 128, 8, 15, 512  # the aw shape of profiles/aw_imaging_n2400.jsonl


def timed(fn, reps, warmup):
    """device milliseconds of fn() per call: warm-up calls, then `reps` calls each between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def split(ctx, fn, reps):
    """gridhip_timing of `reps` further calls: (transform, gather) medians"""
    ctx.enable_timing(True)
    for _ in range(reps):
        fn()
    tr = [ctx.timing(b)[1] for b in range(reps)]
    ga = [ctx.timing(b)[2] for b in range(reps)]
    ctx.enable_timing(False)
    return {"transform_median_ms": statistics.median(tr), "gather_median_ms": statistics.median(ga)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_n2400.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0x9E3779B9)
    uni = lambda lo, hi: torch.rand(n, dtype=torch.float64, device=dev, generator=g) * (hi - lo) + lo
    u, v = uni(-0.45, 0.45) * LAM, uni(-0.45, 0.45) * LAM
    w = uni(-0.5, 0.5) * 20 * KO["wstep"]  # 21 planes of the w_cache rule
    vis = torch.complex(torch.randn(n, dtype=torch.float64, device=dev, generator=g),
                        torch.randn(n, dtype=torch.float64, device=dev, generator=g))
    model = torch.randn((N, N), dtype=torch.float64, device=dev, generator=g)
    kv = bench.synth_kernels(1, 8, 7, dev)[0]  # [Q][Q][7][7]
    # aw: the baseline-structured stream of bench.py (uv as grid fractions, w-bins), uvw in wavelengths here with
    # w = the plane's own w-value, so that findClosest returns the stream's bin
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
    out = torch.empty(n, dtype=torch.complex128, device=dev)
    for name, (uvw, imgfn, b1, b2, vs) in kinds.items():
        fp = lambda: ctx.predict(THETA, LAM, uvw, model, imgfn, a1=b1, a2=b2, out=out)
        fr = lambda: ctx.predict(THETA, LAM, uvw, model, imgfn, a1=b1, a2=b2, vis_sub=vs, out=out)
        fi = lambda: ctx.do_imaging(THETA, LAM, uvw, b1, b2, None, None, vs, imgfn)
        p = timed(fp, args.reps, args.warmup)
        rec(f"predict_dev {name}", p, **split(ctx, fp, args.reps), nonzero=int(torch.count_nonzero(out).item()))
        rec(f"predict_dev {name}, residual form", timed(fr, args.reps, args.warmup))
        d = timed(fi, args.reps, args.warmup)
        rec(f"do_imaging{'_aw' if imgfn[0] == 'aw' else ''}_dev {name}", d,
            predict_over_do_imaging=p["median_ms"] / d["median_ms"])
        if imgfn[0] == "w_cache":
            rec(f"major cycle do_imaging_dev + predict_dev {name}", timed(lambda: (fi(), fp()), args.reps, args.warmup),
                w_range_mirrored=[float(torch.where(v < 0, -w, w).min()), float(torch.where(v < 0, -w, w).max())],
                w_range=[float(w.min()), float(w.max())])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
