#!/usr/bin/env python3
"""Source finding at N = 2400 (the driver's image size) on the three images of tools/automask_timing.py - noise only, noise
plus 300 Gaussian islands, and one all-set component (a constant above fixed levels): gridhip_find_sources_dev (nsigma 5 /
2.5 of the image's own sigma, min_cells 4, a 3-cell beam, the truncation correction, 4096 rows) eagerly and replayed from a
captured graph, next to gridhip_automask_dev (the same levels, grow 2) on the same image, with their ratio.  The all-set
image is the worst case of the measuring kernel: one island whose box is the whole image, walked by one work-group.
Every image is a process of its own under `timeout`, and the steps are chained: a step that fails, faults or runs out of
time ends the run, and nothing more is started on the device.
usage: python tools/sources_timing.py [--reps 5] [--out profiles/sources_n2400.jsonl]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from automask_timing import AM, N, graphed, images, timed  # noqa: E402

THETA, LAM = 0.08, 30000  # image_size = 2400
STEPS = [("noise", 300), ("islands", 300), ("all_set", 300)]
ROWS = 4096
FWHM = 3.0  # the beam, in cells
DEBLEND = [0, 2, 8]  # the window radii of the option "sources_deblend" that are timed; 0 = off


def step(name, reps):
    import torch
    import gridhip
    dev = torch.device("cuda:0")
    ctx = gridhip.Context(0)
    assert ctx.image_size(THETA, LAM) == N
    img = images(torch, dev)[name]
    a = 4.0 * math.log(2.0) / FWHM ** 2
    beam = torch.tensor([a, 0.0, a, FWHM, FWHM, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
    mask = torch.zeros((N, N), dtype=torch.uint8, device=dev)
    out = torch.zeros((ROWS, 10), dtype=torch.float64, device=dev)
    ist = ctx.image_stats(img)
    levels = dict(nsigma=(5, 2.5), noise=ist[3:4]) if name != "all_set" else dict(nsigma=0, thr=(0.5, 0.25))
    src = dict(levels, min_cells=AM["min_cells"], correct=True, max_sources=ROWS, out=out)
    am = dict(levels, min_cells=AM["min_cells"], grow=AM["grow"])
    row = {"what": "find_sources", "image": name, "N": N, "device": torch.cuda.get_device_name(0), "rows": ROWS,
           "options": {k: v for k, v in src.items() if k not in ("noise", "out")}}
    find = lambda: ctx.find_sources(THETA, LAM, img, beam, **src)  # noqa: E731
    mk = lambda: ctx.automask(img, mask, **am)  # noqa: E731
    row["find_sources_eager"] = timed(torch, find, lambda: None, reps)
    graph, (_, count, info, st) = graphed(torch, find)
    row["find_sources_graph"] = timed(torch, graph.replay, lambda: None, reps)
    row["stats"] = st.cpu().tolist()
    written = int(row["stats"][4])
    row["island_cells"] = float(info[:written, 1].sum().item())
    row["largest_island_cells"] = float(info[:written, 1].max().item()) if written else 0.0
    row["automask_eager"] = timed(torch, mk, mask.zero_, reps)
    graph, _ = graphed(torch, mk)
    row["automask_graph"] = timed(torch, graph.replay, mask.zero_, reps)
    row["find_sources_over_automask_graph"] = row["find_sources_graph"]["median_ms"] / row["automask_graph"]["median_ms"]
    row["find_sources_over_automask_eager"] = row["find_sources_eager"]["median_ms"] / row["automask_eager"]["median_ms"]
    rows = [row]
    for r in DEBLEND:  # the same call with the option "sources_deblend" at r (0: the figures above, taken again)
        split = lambda: ctx.find_sources(THETA, LAM, img, beam, deblend=r, **src)  # noqa: E731
        d = {"what": "find_sources_deblend", "image": name, "N": N, "device": row["device"], "rows": ROWS, "deblend": r}
        d["eager"] = timed(torch, split, lambda: None, reps)
        # (the option is read when a call is enqueued, and `deblend` puts it back itself: the capture records the six launches)
        graph, (_, count, info, st) = graphed(torch, split)
        d["graph"] = timed(torch, graph.replay, lambda: None, reps)
        d["stats"] = st.cpu().tolist()
        written = int(d["stats"][4])
        d["blended_rows"] = int((info[:written, 15].to(torch.int64) & 8).ne(0).sum().item())
        d["graph_over_off"] = d["graph"]["median_ms"] / row["find_sources_graph"]["median_ms"]
        rows.append(d)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sources_n2400.jsonl"))
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
