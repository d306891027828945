#!/usr/bin/env python3
"""A set of timing tools on a previous build of the library (tools/ab/libgridhip_prev.so, built as README.md here says) and
on the tree's, in the order previous, tree, tree, previous, in one job on one box.
  --set delay   tools/fringe_timing.py and tools/tec_timing.py       -> profiles/delay_common_ab.jsonl
  --set gain    tools/gaincal_timing.py, tools/ddcal_timing.py and tools/jonescal_timing.py -> profiles/gain_common_ab.jsonl
Every row the tools write goes to --out with three fields added: `library` ("parent" or "tree"), `run` (1..4) and `tool`.
Then the band test, timing by timing.  A timing is a dict with `median_ms`, `min_ms` and `max_ms`: a delay tool's row is one
itself (its key: the tool, `what` and `case`), a gain tool's row holds several by name (`solve_K`, `solve_2K`, `apply`, ...;
their key: the tool, the row's scalars that name the case - `solver`, `n`, `A`, `T`, `D`, `mode`, `path`, `what` - and the
name).  The torch timings are yardsticks and are not judged.  The tree's median of either run must lie within the parent's
median - of its two runs' medians, so their midpoint - plus or minus the distance between those two medians, or, where that
is smaller, the larger max_ms - min_ms of the parent's two runs.
A tool that fails ends the job at once: nothing more is started on the device.  Exit status 1: a timing lies outside.
usage: python tools/ab/delay_ab.py [--set delay] [--out profiles/<set>_common_ab.jsonl] [--reps 5]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PREV = os.path.join(HERE, "libgridhip_prev.so")
SETS = {"delay": ("fringe_timing.py", "tec_timing.py"),
        "gain": ("gaincal_timing.py", "ddcal_timing.py", "jonescal_timing.py")}
NAMES = ("solver", "n", "A", "T", "D", "mode", "path", "what")  # the scalars of a gain tool's row that name its case
TIMING = ("median_ms", "min_ms", "max_ms")


def timings(row):
    """-> [(key, timing)] of one written row: the row itself, or the timing dicts it holds"""
    if all(k in row for k in TIMING):
        return [] if row["what"] == "torch" else [((row["tool"], row["what"], row["case"]), row)]
    case = " ".join(f"{k}={row[k]}" for k in NAMES if k in row)
    return [((row["tool"], case, name), t) for name, t in row.items()
            if isinstance(t, dict) and all(k in t for k in TIMING) and not name.startswith("torch")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default="delay")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"{args.set}_common_ab.jsonl")
    if not os.path.exists(PREV):
        sys.exit(f"{PREV} is missing: build the previous commit's library first (tools/ab/README.md)")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for run, lib in enumerate(("parent", "tree", "tree", "parent"), 1):
            for tool in SETS[args.set]:
                env = dict(os.environ)
                env.pop("GRIDHIP_LIB", None)
                if lib == "parent":
                    env["GRIDHIP_LIB"] = PREV
                part = os.path.join(tmp, f"{run}_{tool}.jsonl")
                print(f"== run {run}: {tool} on the {lib}'s library", flush=True)
                r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.join(ROOT, "tools", tool), "--reps",
                                    str(args.reps), "--out", part], env=env, stdout=subprocess.DEVNULL)
                if r.returncode != 0:
                    sys.exit(f"{tool} ended with status {r.returncode}: nothing more is started")
                with open(part) as f:
                    rows += [dict(library=lib, run=run, tool=tool, **json.loads(line)) for line in f]
    with open(out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    keys = {}
    for r in rows:
        for key, t in timings(r):
            keys.setdefault(key, {"parent": [], "tree": []})[r["library"]].append(t)
    outside = 0
    for (tool, what, case), by in keys.items():
        par = by["parent"]
        pm = [t["median_ms"] for t in par]
        centre, spread = 0.5 * (pm[0] + pm[1]), abs(pm[0] - pm[1])
        band = max(spread, max(t["max_ms"] - t["min_ms"] for t in par))
        new = [t["median_ms"] for t in by["tree"]]
        ok = all(abs(m - centre) <= band for m in new)
        outside += not ok
        if args.set != "delay":
            what = f"{tool[:-10]} {what}"
        print(f"{what:18s} {case[:36]:36s} parent {pm[0]:9.4f} {pm[1]:9.4f} | tree {new[0]:9.4f} {new[1]:9.4f} | "
              f"{centre:9.4f} +- {band:.4f}  {'inside' if ok else 'OUTSIDE'}", flush=True)
    print("rows outside:", outside)
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
