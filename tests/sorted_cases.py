"""Inputs that test_sorted_cases_host.py (host) and test_gpu_sorted_matrix.py (GPU) share: the shapes of the
instantiation matrix of tile_grid_sorted_kernel (csrc/tile_sorted.hip) and streams built so that the walker's control
flow - runs found by ballot, (run, part) units over three tap sets, the pair path, the per-block extra taps, walker
pieces, items and batches - is reached on purpose.  No GPU and no library: plain numpy.  The host test shows that every
stream has the structure it is named for and that the integer streams are exact in fp64.

Coordinates.  oracle/gridref_np.frac_coord: x = n // 2 + p * n, cell = floor(x + 0.5 / Q), fraction = round((x - cell)
* Q).  A record at cell c with fraction f therefore has p = (c + f / Q - n // 2) / n (`at_cells`); u runs along the
columns (Wd), v along the rows (H).  A record's kernel slice is (wbin * Q + yf) * Q + xf; the tile kernel sorts a work
item's records by it, so a RUN is a stretch of equal slice in the slice-sorted order of one (w-group, tile) item.
The tile of a record is that of its footprint origin (cell - S // 2), floor-divided by the tile's interior."""
from collections import namedtuple

import numpy as np

SUPPORTS = tuple(range(5, 33))          # every support the kernel is instantiated for
AW_SUPPORTS = tuple(range(5, 17))       # ... in its aw form

# B1 / B2: a non-square grid with footprints spilling over all four edges
H1, WD1, N1, SPREAD1 = 192, 224, 30000, 0.6
DENSITIES = {"long": (2, 2), "short": (4, 8)}   # name -> (W, Q)
SMALL_TILE = 16                          # what a grid this small gets by default: the tile shrinks to 16 x 16

# B2: the tile a large grid gets for each support (last_tile_x, last_tile_y on a grid of >= 1024 such tiles, W = Q = 2).
# The GPU test probes the library and compares with this table, so a change of the geometry rule is noticed.
# DESIGN.md's 65 x 89 at 15 x 15 is the one value known beforehand; the others follow from the same rule (the widest tile
# of each row pitch, the tallest height whose plane stays below the fixed re / im distance of 65528 bytes).
PROD_TILE = {5: (97, 77), 6: (65, 112), 7: (65, 109), 8: (65, 106), 9: (97, 70), 10: (97, 68), 11: (65, 99),
             12: (65, 96), 13: (97, 63), 14: (65, 92), 15: (65, 89), 16: (65, 87), 17: (65, 85), 18: (65, 82),
             19: (65, 80), 20: (65, 78), 21: (65, 76), 22: (65, 74), 23: (65, 72), 24: (65, 70), 25: (65, 68),
             26: (65, 66), 27: (65, 64), 28: (65, 62), 29: (65, 60), 30: (65, 58), 31: (65, 56), 32: (65, 54)}

# B3: one grid with room for 1024 big tiles
N3, W3, Q3 = 3200, 2, 2
# supports for which option "bigtile" = 1 yields last_bigtile = 1 on that grid (recorded from the library; the existing
# tests establish 9, 15, 17 and 21)
BIGTILE_SUPPORTS = frozenset(range(5, 33))

# B4: the aw form
H4, WD4, N4, W4, Q4, A4 = 96, 112, 6000, 2, 2, 3

# C: representatives of every compile-time class
CLASS_SUPPORTS = (5, 8, 15, 16, 17, 18, 23, 31, 32)
AW_CLASS_SUPPORTS = (5, 15, 16)
HC, WDC = 192, 224                       # the grid of the structured streams
CELL = (100, 90)                         # (column, row) of the one cell most streams sit at: footprints inside the grid
VMAX = 3                                 # integer values in -VMAX .. VMAX


def shape_class(S, degrid):
    """The compile-time shape of tile_grid_sorted_kernel<S, DEGRID>, restated from its constexprs: steps the tap list
    is taken in, taps of the last step, per-block extra taps, the pair path, parts of the tap list and their steps."""
    S2 = S * S
    tail0 = S2 - ((S2 + 63) // 64 - 1) * 64
    extra = 0 if degrid else tail0 - 32 if 32 < tail0 <= 34 else tail0 if S2 > 256 and tail0 <= 2 else 0
    s2e = S2 - extra
    nstep = (s2e + 63) // 64
    tail = s2e - (nstep - 1) * 64
    maxst = 4 if degrid else 5
    fp = (nstep + maxst - 1) // maxst
    kst = (nstep + fp - 1) // fp
    return dict(steps=nstep, tail=tail, extra=extra, pair=(not degrid) and tail == 32, parts=fp, kst=kst, rem=nstep % fp)


def at_cells(H, Wd, Q, cx, cy, xf, yf):
    """(u, v) of records at cells (cx, cy) with sub-cell fractions (xf, yf) / Q"""
    cx, cy, xf, yf = (np.asarray(a, dtype=np.float64) for a in (cx, cy, xf, yf))
    return (cx + xf / Q - Wd // 2) / Wd, (cy + yf / Q - H // 2) / H


def slices_of(H, Wd, Q, u, v, wb):
    """(kept, cell x, cell y, slice) per record, by the reference's coordinate rule; kept = finite and 0 <= wb (the
    caller bounds wb from above)"""
    from oracle import gridref_np as P
    ok = np.isfinite(u) & np.isfinite(v) & (np.asarray(wb) >= 0)
    x, xf, y, yf = P.frac_coords((H, Wd), Q, np.where(ok, u, 0.0), np.where(ok, v, 0.0))
    return ok, x, y, (np.asarray(wb) * Q + yf) * Q + xf


def run_lengths(keys):
    """lengths of the stretches of equal key in the sorted order of `keys`"""
    return np.unique(np.asarray(keys), return_counts=True)[1]


def mean_run_length(H, Wd, W, Q, S, tile, u, v, wb):
    """records per (tile, slice) among the pairs that occur, for the visibilities with a tap inside the grid; one
    w-group (W < 8), tile = (Tx, Ty)"""
    ok, x, y, sl = slices_of(H, Wd, Q, u, v, wb)
    x0, y0 = x - S // 2, y - S // 2
    ok &= (wb < W) & (x0 + S > 0) & (y0 + S > 0) & (x0 < Wd) & (y0 < H)
    tx, ty = np.floor_divide(x0, tile[0]), np.floor_divide(y0, tile[1])
    pair = ((ty[ok] + 64) * 4096 + tx[ok] + 64) * (W * Q * Q) + sl[ok]
    return ok.sum() / len(np.unique(pair))


# ---- B: seeded streams ------------------------------------------------------------------------------------------------
def uniform_case(seed, H, Wd, W, Q, S, n, spread):
    rng = np.random.default_rng(seed)
    gcf = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    u, v = rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n)
    wb = rng.integers(0, W, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    return gcf, u, v, wb, vis


def window_case(seed, S, n=N1):
    """B3: half the visibilities in a window of 3 x 3 big tiles (about 290 cells a side) that touches the grid's corner -
    footprint origins from outside the grid to inside it - and half in one at the centre"""
    rng = np.random.default_rng(seed)
    gcf = rng.normal(size=(W3, Q3, Q3, S, S)) + 1j * rng.normal(size=(W3, Q3, Q3, S, S))
    side, h = 290, n // 2
    cx = np.concatenate([rng.uniform(0.6 - (S - 1) // 2, side, h), rng.uniform(N3 // 2 - side / 2, N3 // 2 + side / 2, n - h)])
    cy = np.concatenate([rng.uniform(0.6 - (S - 1) // 2, side, h), rng.uniform(N3 // 2 - side / 2, N3 // 2 + side / 2, n - h)])
    u, v = (cx - N3 // 2) / N3, (cy - N3 // 2) / N3
    wb = rng.integers(0, W3, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    return gcf, u, v, wb, vis, side


def aw_case(seed, H, Wd, W, Q, S, A, n, spread=0.5):
    rng = np.random.default_rng(seed)
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    u, v = rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n)
    wb, a1, a2 = rng.integers(0, W, n), rng.integers(0, A, n), rng.integers(0, A, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    G = rng.normal(size=(H, Wd)) + 1j * rng.normal(size=(H, Wd))
    return wk, ak, u, v, wb, a1, a2, vis, G


# ---- C: structured streams, small integers ---------------------------------------------------------------------------
# opts: options the stream needs on top of the geometry's; ndrop: records that must come back as exact zeros
Stream = namedtuple("Stream", "name W Q u v wb opts ndrop")


def cint(rng, shape):
    """complex values with integer parts in -VMAX .. VMAX"""
    return (rng.integers(-VMAX, VMAX + 1, shape) + 1j * rng.integers(-VMAX, VMAX + 1, shape)).astype(np.complex128)


def int_tables(S, W, Q, n, seed=0):
    """(gcf, vis, G): integer kernel taps, visibilities and degrid input grid for a stream of n records"""
    rng = np.random.default_rng(1000 * S + 10 * W + Q + seed)
    return cint(rng, (W, Q, Q, S, S)), cint(rng, n), cint(rng, (HC, WDC))


def _from_slices(name, W, Q, sl, cx=None, cy=None, opts=None, drops=0, seed=0):
    """records of slices `sl` (any order) at CELL (or cells cx, cy); `drops` = 3 appends two NaN coordinates and one
    wbin = W"""
    sl = np.asarray(sl, dtype=np.int64)
    wb, yf, xf = sl // (Q * Q), (sl // Q) % Q, sl % Q
    n = len(sl)
    cx = np.full(n, CELL[0]) if cx is None else np.asarray(cx)
    cy = np.full(n, CELL[1]) if cy is None else np.asarray(cy)
    u, v = at_cells(HC, WDC, Q, cx, cy, xf, yf)
    if drops:
        assert drops == 3
        rng = np.random.default_rng(seed)
        pos = np.sort(rng.choice(n, 3, replace=False))
        u, v, wb = (np.insert(a, pos, a[pos]) for a in (u, v, wb))   # three more records, copies of their neighbours
        k = pos + np.arange(3)
        u[k[0]], v[k[1]], wb[k[2]] = np.nan, np.nan, W
    return Stream(name, W, Q, u, v, wb.astype(np.int64), dict(opts or {}), drops)


ONE_RUN_LENGTHS = (1, 2, 3, 63, 64, 65, 129, 1000)


def one_run(n):
    """1. n records of one slice at one cell"""
    return _from_slices(f"one_run_{n}", 2, 2, np.full(n, 6))   # (wb, yf, xf) = (1, 1, 0)


def singles():
    """2. runs of length 1 only: W = 4, Q = 8, one w-group, every one of the 256 slices once, in a shuffled order"""
    return _from_slices("singles", 4, 8, np.random.default_rng(2).permutation(256), drops=3, seed=2)


LADDER = 24


def ladder(reverse):
    """3. runs of length 1, 2, .. 24 in slice order (300 records), or 24 .. 1; the records arrive shuffled"""
    lens = np.arange(1, LADDER + 1)[::-1] if reverse else np.arange(1, LADDER + 1)
    sl = np.repeat(np.arange(LADDER), lens)
    return _from_slices("ladder_down" if reverse else "ladder_up", 2, 4, np.random.default_rng(3).permutation(sl), drops=3,
                        seed=3 + reverse)


FEW_CELLS = ((20, 20), (200, 20), (20, 170), (200, 170))   # four tiles under every geometry used (host test)


def few(k):
    """4. fewer records than walkers: items of 1 + k, 5 + k, 9 + k, 13 + k records (k = 0..3: every size 1..16) in four
    tiles of one call"""
    sizes = [1 + k, 5 + k, 9 + k, 13 + k]
    cx = np.repeat([c[0] for c in FEW_CELLS], sizes)
    cy = np.repeat([c[1] for c in FEW_CELLS], sizes)
    sl = np.random.default_rng(40 + k).integers(0, 8, len(cx))
    return _from_slices(f"few_{k}", 2, 2, sl, cx, cy)


BATCH_LENGTHS = (64, 65, 128, 129)


def batches(n):
    """5. items and batches: "chunk" = 64 with n records in one tile"""
    return _from_slices(f"batches_{n}", 2, 2, np.random.default_rng(50 + n).integers(0, 8, n), opts={"chunk": 64})


def window(tile, S):
    """6. one visibility at every cell of a window of (Tx + 2) x (Ty + 2) cells, one slice: every footprint position a
    tile can hold, whatever the tile's origin"""
    nx, ny = tile[0] + 2, tile[1] + 2
    assert 40 + nx + S // 2 < WDC and 30 + ny + S // 2 < HC
    cx, cy = np.meshgrid(40 + np.arange(nx), 30 + np.arange(ny))
    return _from_slices(f"window_{tile[0]}x{tile[1]}", 2, 2, np.full(nx * ny, 3), cx.ravel(), cy.ravel())


WGROUP_CASES = ((5, 3), (13, 16))


def wgroups(W, ng):
    """7. w-groups that do not divide W: 2000 records at one cell cycling through all planes and fractions"""
    return _from_slices(f"wgroups_{W}_{ng}", W, 2, np.arange(2000) % (W * 4), opts={"wgroups": ng})


def structured_streams():
    """streams 1 - 5 and 7 (6 depends on the tile and is built by the caller)"""
    out = [one_run(n) for n in ONE_RUN_LENGTHS] + [singles(), ladder(False), ladder(True)]
    out += [few(k) for k in range(4)] + [batches(n) for n in BATCH_LENGTHS] + [wgroups(W, ng) for W, ng in WGROUP_CASES]
    return out


def int_eval(gcf, H, Wd, u, v, wb, vis=None, G=None):
    """convgrid2 (vis given) or degrid2 (G given) of integer-valued inputs in int64 - no floating point after the
    coordinates.  Dropped: non-finite coordinates and wb outside [0, W).  Returns (re, im, largest |partial sum|
    bound): the bound is the sum of |products| per output element, which no partial sum in any order can exceed."""
    W, Q, _, S, _ = gcf.shape
    ok, x, y, sl = slices_of(H, Wd, Q, u, v, wb)
    ok &= np.asarray(wb) < W
    kr, ki = (np.rint(a).astype(np.int64).reshape(W * Q * Q, S, S) for a in (gcf.real, gcf.imag))
    idx = np.flatnonzero(ok)
    x0, y0, sl = x[idx] - S // 2, y[idx] - S // 2, sl[idx]
    if vis is not None:
        vr, vi = np.rint(vis.real).astype(np.int64)[idx], np.rint(vis.imag).astype(np.int64)[idx]
        outr, outi, mag = (np.zeros((H, Wd), dtype=np.int64) for _ in range(3))
    else:
        gr, gi = np.rint(G.real).astype(np.int64), np.rint(G.imag).astype(np.int64)
        outr, outi, mag = (np.zeros(len(u), dtype=np.int64) for _ in range(3))
    for i in range(S):
        for j in range(S):
            xx, yy = x0 + j, y0 + i
            m = (xx >= 0) & (yy >= 0) & (xx < Wd) & (yy < H)
            a, b = kr[sl[m], i, j], ki[sl[m], i, j]
            if vis is not None:
                np.add.at(outr, (yy[m], xx[m]), vr[m] * a - vi[m] * b)
                np.add.at(outi, (yy[m], xx[m]), vr[m] * b + vi[m] * a)
                np.add.at(mag, (yy[m], xx[m]), (np.abs(vr[m]) + np.abs(vi[m])) * (np.abs(a) + np.abs(b)))
            else:
                c, d = gr[yy[m], xx[m]], gi[yy[m], xx[m]]
                outr[idx[m]] += a * c - b * d
                outi[idx[m]] += a * d + b * c
                mag[idx[m]] += (np.abs(a) + np.abs(b)) * (np.abs(c) + np.abs(d))
    return outr, outi, int(mag.max())


# ---- C 8: aw residues ------------------------------------------------------------------------------------------------
AW8 = dict(S=15, A=12, W=5, Q=4, n=12000)   # 12 * 12 * 5 * 4 * 4 = 11 520 possible kernels (A = 9 would give 6 480 < 8 192)
AW_KEYS = 4096                               # the aw sort is by kernel index mod 4096 (sorted_plan)


def aw_residues():
    """8. one batch, every record at one cell of the B4 grid (so one tile), 12 000 records over at least 8 192 distinct
    (a1, a2, wbin, yf, xf) kernels: the first 11 520 records take every kernel once, the rest repeat some.  The device
    numbers a batch's distinct kernels 0 .. D - 1, so with D >= 8192 every one of the 4096 histogram slots holds two
    kernels or more, which interleave in the sorted list."""
    S, A, W, Q, n = (AW8[k] for k in ("S", "A", "W", "Q", "n"))
    rng = np.random.default_rng(8)
    total = A * A * W * Q * Q
    key = np.concatenate([rng.permutation(total), rng.integers(0, total, n - total)])[:n]
    a1, a2, wb, yf, xf = np.unravel_index(key, (A, A, W, Q, Q))
    u, v = at_cells(H4, WD4, Q, np.full(n, 50), np.full(n, 44), xf, yf)
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    G = rng.normal(size=(H4, WD4)) + 1j * rng.normal(size=(H4, WD4))
    return wk, ak, u, v, wb.astype(np.int64), a1.astype(np.int64), a2.astype(np.int64), vis, G
