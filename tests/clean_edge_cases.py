"""Inputs that test_clean_edges_host.py (host) and test_gpu_clean_edges.py (GPU) share: the fixtures at which the three
minor-cycle loops (clean.hip, msclean.hip, mfclean.hip) meet ties, the image's rim, tiny images and misaligned bases.
No GPU: plain numpy and the restatements clean_ref, msclean_ref, mfclean_ref and clean_auto_ref.

Exact fixtures.  The PSF's cells are signed powers of two (1.0 at the centre, 2^-1 .. 2^-3 elsewhere, sign and exponent
by position so that a read of the wrong PSF cell shows), the residual's cells are small integers, gain is 0.5 or 0.25
and the threshold 0: every product and every difference of a run is then exact in fp64, and a correct kernel gives the
restatement's BITS whatever it fuses.  Where patch > 0 keeps the tied cells out of each other's update region the equal
maxima stay exactly equal from iteration to iteration; a patch = 0 fixture meets its tie on the first pick only (the
first subtraction reaches the other cell).  That every operation
was exact is not argued but checked, by the host test: the same run in np.longdouble gives the same numbers.

The tile geometry the placements refer to: tiles of TH = 16 rows x TW = 128 columns, table entry ty * ntx + tx; in a tile
kernel wave w takes rows w, w + 4, w + 8, w + 12 and a lane the two cells of one 16-byte slot; the pick kernel's thread t
takes entries t, t + 1024, t + 2048 and its wave t // 64 reduces them."""
import functools
from collections import namedtuple

import numpy as np

import clean_auto_ref
import clean_ref
import mfclean_ref
import msclean_ref

TH, TW = 16, 128
LOOPS = ("clean", "ms0", "mf1")  # Hogbom, msclean with scales = [0], mfclean with T = 1: the same numbers, three tile codes

# name; N; cells: (y, x, value) laid over the fill; fill: "noise" (-1 or 1 by a seeded draw), "zero", "nan", "nanrim" (NaN outside
# the border, noise inside) or a number; mask: cells (y, x) whose mask byte is 0, or None (no mask: the plain entry point)
Fx = namedtuple("Fx", "name N cells fill gain niter border patch mask")


def fx(name, N, cells, fill="noise", gain=0.5, niter=5, border=0, patch=0, mask=None):
    return Fx(name, N, tuple(cells), fill, gain, niter, border, patch, None if mask is None else tuple(mask))


@functools.lru_cache(maxsize=4)
def exact_psf(N):
    """1.0 at (N // 2, N // 2); elsewhere +-2^-(1 + (3 dy + 5 dx) mod 3), negative where (dy * dx + dy) mod 3 == 0"""
    c = N // 2
    dy, dx = np.mgrid[0:N, 0:N] - c
    psf = np.ldexp(1.0, -(1 + (3 * dy + 5 * dx) % 3)) * np.where((dy * dx + dy) % 3 == 0, -1.0, 1.0)
    psf[c, c] = 1.0
    psf.setflags(write=False)
    return psf


def residual_of(f):
    N = f.N
    if f.fill in ("noise", "nanrim"):
        res = np.random.default_rng(7 * N + 1).integers(0, 2, (N, N)).astype(np.float64) * 2.0 - 1.0
        if f.fill == "nanrim":
            inner = np.zeros((N, N), dtype=bool)
            inner[f.border:N - f.border, f.border:N - f.border] = True
            res[~inner] = np.nan
    else:
        res = np.full((N, N), {"zero": 0.0, "nan": np.nan}.get(f.fill, f.fill), dtype=np.float64)
    for y, x, v in f.cells:
        res[y, x] = v
    return res


def mask_of(f):
    if f.mask is None:
        return None
    m = np.ones((f.N, f.N), dtype=np.uint8)
    for y, x in f.mask:
        m[y, x] = 0
    return m


def reference(loop, f, dtype=np.float64, trace=None):
    """(model, residual, stats) of fixture f by the loop's own restatement, on arrays of `dtype`.  A fixture with a mask
    takes the _auto restatement (clean only)."""
    psf, res = exact_psf(f.N).astype(dtype), residual_of(f).astype(dtype)
    model = np.zeros_like(res)
    g, n, b, p = dtype(f.gain), f.niter, f.border, f.patch
    with np.errstate(invalid="ignore"):
        if f.mask is not None:
            assert loop == "clean"
            stats = clean_auto_ref.clean(psf, res, model, g, 0.0, n, b, p, mask=mask_of(f), trace=trace)
        elif loop == "clean":
            stats = clean_ref.clean(psf, res, model, g, 0.0, n, b, p, trace)
        elif loop == "ms0":
            stats = msclean_ref.msclean(psf, res, model, [0.0], [1.0], g, 0.0, n, b, p, trace=trace)
        else:
            stats = mfclean_ref.mfclean(psf[None], res[None], model[None], g, 0.0, n, b, p, trace)
    return model, res, stats


def mutant(f, highest=False, clip=1, dtype=np.float64):
    """(residual, component sequence) of clean_ref.clean with one statement changed.  highest: peak() takes the HIGHEST
    flat index among equal maxima.  clip = 2: the update region ends at N - 2 instead of N - 1.  Neither changed: the
    restatement itself, mask included (the host test checks that), which is how a masked fixture is rerun in
    np.longdouble: clean_auto_ref's exact fma takes Python floats only."""
    psf, res = exact_psf(f.N).astype(dtype), residual_of(f).astype(dtype)
    mask = mask_of(f)
    N, c, b = f.N, f.N // 2, f.border
    seq = []
    for _ in range(f.niter):
        a = np.abs(res[b:N - b, b:N - b])
        a = np.where(np.isnan(a), -1.0, a)
        if mask is not None:
            a = np.where(mask[b:N - b, b:N - b] != 0, a, -1.0)
        j = a.size - 1 - int(np.argmax(a[::-1, ::-1])) if highest else int(np.argmax(a))
        if not a.flat[j] > 0:
            break
        y, x = divmod(j, a.shape[1])
        y, x = y + b, x + b
        seq.append(y * N + x)
        g = dtype(f.gain) * res[y, x]
        ylo, yhi, xlo, xhi = max(0, y - c), min(N - clip, y - c + N - 1), max(0, x - c), min(N - clip, x - c + N - 1)
        if f.patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - f.patch), min(yhi, y + f.patch), max(xlo, x - f.patch), min(xhi, x + f.patch)
        if yhi >= ylo and xhi >= xlo:
            res[ylo:yhi + 1, xlo:xhi + 1] -= g * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
    return res, seq


def same_bits(a, b):
    """equal as bits: NaN where NaN (whatever its sign and payload), and the sign of a zero counts"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    return np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


# ---- 2. tie placements -----------------------------------------------------------------------------------------------------
def slot_x(N, y, x):
    """the even-address cell of a slot near x in row y (the arrays of a plain run are 16-byte aligned)"""
    return x + (y * N + x) % 2


def tie_fixtures():
    out = []
    for N in (257, 300):
        t = lambda name, cells, **kw: out.append(fx(f"{name}-N{N}", N, [(y, x, 3.0) for y, x in cells], **kw))  # noqa: E731
        x = slot_x(N, 20, 10)
        t("a-slot-even-row", [(20, x), (20, x + 1)])
        x = slot_x(N, 21, 10)
        t("a-slot-odd-row", [(21, x), (21, x + 1)])
        t("a-neighbours-in-two-tiles", [(20, 255), (20, 256)])
        t("b-lanes-0-63", [(33, 0), (33, 126)], patch=1, gain=0.25)
        t("b-lanes-0-63-second-tile", [(33, 128), (33, 254)], patch=1, gain=0.25)
        t("c-rows-r-r4-lanes", [(18, 100), (22, 4)], patch=1, gain=0.25)
        t("c-rows-r-r4-one-column", [(35, 7), (39, 7)], patch=1, gain=0.25)
        t("d-rows-4-1", [(17, 50), (20, 20)])
        t("d-rows-4-1-patch", [(17, 50), (20, 20)], patch=1, gain=0.25)
        t("e-later-entry-lower-index", [(0, 130), (1, 5)], patch=1, gain=0.25)
        t("e-later-entry-lower-index-full", [(0, 130), (1, 5)])
        t("e-two-tile-rows", [(15, 140), (16, 2)], patch=1, gain=0.25)
        t("e-last-tile-column", [(40, N - 1), (41, 0)], patch=1, gain=0.25)
    for N in (129, 130, 257):
        out.append(fx(f"g-sign-of-the-lower-N{N}", N, [(5, 7, -3.0), (9, 3, 3.0)], patch=1, gain=0.25, niter=3))
        out.append(fx(f"g-sign-in-one-slot-N{N}", N, [(6, slot_x(N, 6, 8), -3.0), (6, slot_x(N, 6, 8) + 1, 3.0)], niter=3))
        out.append(fx(f"h-constant-border-N{N}", N, [], fill=3.0, border=3, niter=3))
        out.append(fx(f"h-constant-masked-N{N}", N, [], fill=3.0, border=3, niter=3, mask=[(3, 3 + i) for i in range(5)]))
    return out


# (f) N = 2049: 17 x 129 = 2193 tiles.  Entries 88 and 1112 = 88 + 1024 are one pick thread's first and second trip;
# 144 and 2192 = 144 + 2048 (the 1 x 1 corner tile) its first and third; 700 is reduced by another wave (10) than 88 (1)
# and 144 (2).  Patch 32 keeps the cells from touching each other: the five stay tied, round after round.
BIG_N = 2049


def entry_cell(e, r, xoff, N=BIG_N):
    ntx = (N + TW - 1) // TW
    return (e // ntx) * TH + r, (e % ntx) * TW + xoff


def big_fixture():
    cells = [entry_cell(88, 2, 9), entry_cell(1112, 3, 11), entry_cell(700, 1, 64), entry_cell(144, 5, 127),
             (BIG_N - 1, BIG_N - 1)]
    return fx("f-second-trip-waves-corner-tile-N2049", BIG_N, [(y, x, 3.0) for y, x in cells], gain=0.25, niter=12, patch=32)


# ---- 3. rim and small N ------------------------------------------------------------------------------------------------------
RIM_N = (1, 2, 3, 15, 16, 17, 127, 128, 129, 257)


def rim_cells(N):
    """the four corners and the four edge midpoints (as many as are distinct), magnitudes 5, 6, ... with alternating sign"""
    m, e = N // 2, N - 1
    pos = []
    for p in [(0, 0), (0, e), (e, 0), (e, e), (0, m), (m, 0), (m, e), (e, m)]:
        if p not in pos:
            pos.append(p)
    return [(y, x, (5.0 + i) * (-1.0) ** i) for i, (y, x) in enumerate(pos)]


def rim_fixtures():
    """Every N x patch x border; clean_check refuses none of them.  At N = 1 and N = 2 the border (N - 1) // 2 is 0, the
    same fixture again, and at N = 1 patch = N is patch = 1: each is listed once, 89 fixtures of the 100.  With
    border = (N - 1) // 2 the search window is one or two cells wide and every component lies in the middle: those
    fixtures cover the border-window search, not the clip at the rim (the host test's clip mutant takes border = 0)."""
    out = []
    for N in RIM_N:
        for patch in sorted({0, 1, 64, N, 2 * N}):
            for border in sorted({0, (N - 1) // 2}):
                out.append(fx(f"rim-N{N}-patch{patch}-border{border}", N, rim_cells(N), niter=8, border=border, patch=patch))
    return out


def straddle_fixtures():
    """N = 257.  patch = 1 around x in {127, 128}, y in {15, 16}: a 3 x 3 region over four tiles.  patch = 64 at x = 64 -
    the 129-cell region 0 .. 128 starts on a tile's first cell and ends on the next tile's first - and at x = 191 - it is
    127 .. 255, from a tile's last cell; in y the regions 16 .. 144 and 106 .. 234 overlap nine tile rows each, the most
    tiles_spanned allows for 129 cells.  patch = 65: the partial launch is three tile columns wide; the 131-cell region
    of x = 127 is 62 .. 192, two of them (the third work-group leaves), that of x = 191 is 126 .. 256, all three."""
    return [fx("straddle-patch65-three-tile-columns-N257", 257, [(80, 127, 5.0), (170, 191, -6.0)], niter=4, patch=65),
            fx("straddle-four-tiles-N257", 257, [(15, 127, 5.0), (15, 128, -6.0), (16, 127, 7.0), (16, 128, -8.0)],
               niter=6, patch=1),
            fx("straddle-patch64-N257", 257, [(80, 64, 5.0), (170, 191, -6.0)], niter=4, patch=64)]


# ---- 4. misaligned bases -------------------------------------------------------------------------------------------------------
def misaligned_fixtures():
    out = []
    for N in (128, 129):
        for patch in (0, 5):
            out.append(fx(f"misaligned-N{N}-patch{patch}", N, rim_cells(N) + [(N // 2, N // 2 + 1, 14.0)], niter=6,
                          patch=patch))
            out.append(fx(f"misaligned-masked-N{N}-patch{patch}", N, rim_cells(N) + [(N // 2, N // 2 + 1, 14.0)], niter=6,
                          patch=patch, mask=[(0, 0), (N - 1, N - 1), (N // 2, N // 2 + 1)]))
    return out


# ---- 5. special values: one iteration each -------------------------------------------------------------------------------------
def special_fixtures():
    out = []
    for N in (17, 130):
        out += [fx(f"negative-zero-alone-N{N}", N, [(N // 3, N - 2, -0.0)], fill="nan", niter=1),
                fx(f"denormal-peak-N{N}", N, [(2, N - 1, 3 * 5e-324)], fill="zero", niter=1),
                fx(f"infinities-tied-N{N}", N, [(1, N - 1, -np.inf), (3, 4, np.inf)], niter=1),
                fx(f"nan-outside-the-border-N{N}", N, [(4, 5, 4.0)], fill="nanrim", niter=1, border=2)]
    return out


# ---- 6. the wide forms: msclean with several scales, mfclean with T > 1 ----------------------------------------------------
# These round, so their ties are made by translation: identical stamps on a zero background, further apart than the patch
# and the scale kernels reach and clear of the rim, so that every smoothed residual and every score has the same bits at
# every stamp - in the library's arithmetic and in the restatement's, separately - and stays so while the stamps are
# taken in turn.  kind "ms": scales, bias; kind "mf": T.  cells: (y, x, amplitude); stamp: lay the 3 x 3 STAMP (else the
# one cell) over a zero background (else over seeded noise of 0.01).  ties: the picks whose gap must be exactly 0.
Wide = namedtuple("Wide", "name kind N scales bias T cells stamp gain niter border patch ties")
STAMP = np.array([[0.3, 0.5, 0.2], [0.6, 1.0, 0.4], [0.1, 0.7, 0.35]])
TERM = (1.0, 0.35, -0.15)  # a stamp's amplitude in the residual of term t


@functools.lru_cache(maxsize=8)
def wide_psfs(N, T):
    """2T - 1 spectral PSFs of any N >= 1: P_s = sum_j w_j x_j^s g_j over three smooth shapes g_j with g_j = 1 at the
    centre, so the Hessian P_{t+q}[c, c] is the moment matrix of three points: positive definite up to T = 3.  P_0 is
    1.0 at the centre, its largest cell; wide_psfs(N, 1)[0] is the PSF of the msclean fixtures."""
    c = N // 2
    dy, dx = (np.mgrid[0:N, 0:N] - c).astype(np.float64)
    out = np.zeros((2 * T - 1, N, N))
    for j, (w, x) in enumerate(zip((0.3, 0.4, 0.3), (-0.2, 0.05, 0.25))):
        g = np.exp(-0.5 * (dy * dy + dx * dx) / (1.2 + 0.4 * j) ** 2) * np.cos(0.2 * (j + 1) * dy + 0.15 * j * dx)
        g = (g + 0.02 * np.cos(0.31 * dy - 0.23 * dx + j)) / (1.0 + 0.02 * np.cos(float(j)))
        for s in range(2 * T - 1):
            out[s] += w * x ** s * g
    out /= out[0][c, c]
    assert out[0][c, c] == 1.0 and np.argmax(out[0]) == c * N + c
    out.setflags(write=False)
    return out


def wide(name, kind, N, cells, scales=(0.0, 2.0), bias=None, T=2, stamp=True, gain=0.25, niter=4, border=0, patch=6,
         ties=(0, 2)):
    if kind == "ms":
        bias = tuple(msclean_ref.default_bias(scales)) if bias is None else tuple(bias)
        return Wide(name, kind, N, tuple(scales), bias, 1, tuple(cells), stamp, gain, niter, border, patch, tuple(ties))
    return Wide(name, kind, N, None, None, T, tuple(cells), stamp, gain, niter, border, patch, tuple(ties))


def wide_inputs(w):
    """(psf or psfs, residual or residuals): [N, N] for msclean, [2T - 1, N, N] and [T, N, N] for mfclean"""
    N, T = w.N, w.T
    res = np.zeros((T, N, N)) if w.stamp else 0.01 * np.random.default_rng(11 * N + T).normal(size=(T, N, N))
    for y, x, v in w.cells:
        for t in range(T):
            if w.stamp:
                res[t, y - 1:y + 2, x - 1:x + 2] = v * TERM[t] * STAMP
            else:
                res[t, y, x] = v * TERM[t]
    psfs = np.array(wide_psfs(N, T))
    return (psfs[0], res[0]) if w.kind == "ms" else (psfs, res)


def wide_reference(w):
    """(model, residual, stats, trace) of the wide fixture by its restatement"""
    psf, res = wide_inputs(w)
    model, trace = np.zeros_like(res), []
    if w.kind == "ms":
        stats = msclean_ref.msclean(psf, res, model, list(w.scales), list(w.bias), w.gain, 0.0, w.niter, w.border, w.patch,
                                    trace=trace)
    else:
        stats = mfclean_ref.mfclean(psf, res, model, w.gain, 0.0, w.niter, w.border, w.patch, trace)
    return model, res, stats, trace


# the placements (c), (d), (e) of the exact fixtures, moved clear of the rim and of each other
WIDE_PLACES = {"c-rows-r-r4": [(34, 100), (38, 20)], "d-rows-4-1": [(33, 90), (36, 20)],
               "e-later-entry-lower-index": [(8, 140), (9, 40)], "e-two-tile-rows": [(15, 150), (16, 30)]}
WIDE_KINDS = {"ms2": dict(kind="ms"), "mf2": dict(kind="mf", T=2), "mf3": dict(kind="mf", T=3)}


def wide_tie_fixtures():
    out = []
    for N in (257, 300):
        for kn, kw in WIDE_KINDS.items():
            for pn, cells in WIDE_PLACES.items():
                out.append(wide(f"{kn}-{pn}-N{N}", N=N, cells=[(y, x, 1.0) for y, x in cells], **kw))
    # radius 31: the scale 32; the stamps are rows 2 and 6 of a tile, 160 columns apart
    out.append(wide("ms32-c-rows-r-r4-N257", "ms", 257, [(66, 40, 1.0), (70, 200, 1.0)], scales=(0.0, 32.0)))
    return out


def wide_big_fixtures():
    """N = 2049: stamps in the table entries 88, 700 and 1112 = 88 + 1024.  Pick 0 is a tie of three, pick 1 of 700 and
    1112 - the lower index sits in the pick kernel's wave 10, the higher came to wave 1 on thread 88's second trip -
    pick 2 is 1112 alone, picks 3 and 4 repeat 0 and 1."""
    cells = [entry_cell(88, 2, 9) + (1.0,), entry_cell(700, 1, 64) + (1.0,), entry_cell(1112, 3, 11) + (1.0,)]
    kw = dict(N=BIG_N, cells=cells, patch=32)
    return [wide("ms2-f-second-trip-N2049", "ms", niter=3, ties=(0, 1), **kw),
            wide("mf2-f-second-trip-N2049", "mf", T=2, niter=5, ties=(0, 1, 3, 4), **kw)]


def wide_rim_cells(N):
    """rim_cells with magnitudes 5, 6.13, 7.26, ...: no product of a power of the gain and one of them equals another"""
    return [(y, x, v + 0.13 * i * (1.0 if v > 0 else -1.0)) for i, (y, x, v) in enumerate(rim_cells(N))]


def wide_rim_fixtures():
    out = []
    for N in (1, 2, 3, 17, 129):
        for kn in ("ms2", "mf2"):
            for patch in (0, 1):
                out.append(wide(f"{kn}-rim-N{N}-patch{patch}", N=N, cells=wide_rim_cells(N), stamp=False, gain=0.5, niter=8,
                                patch=patch, ties=(), **WIDE_KINDS[kn]))
    return out


def wide_misaligned_fixtures():
    """even N: plane 0 of the stacks is 8 bytes off only when the base is"""
    return [wide(f"{kn}-misaligned-N128", N=128, cells=wide_rim_cells(128) + [(64, 65, 14.3)], stamp=False, gain=0.5, niter=6,
                 patch=5, ties=(), **WIDE_KINDS[kn]) for kn in ("ms2", "mf2", "mf3")]


# The tie BETWEEN scales.  The scale 1.0 has radius 0: its kernel is the one tap 1.0, so R_1 = R_0 and q_1 = q_0 = 1 with no
# rounding anywhere, in the library as in the restatement.  With bias = [1, 1], b_s (p_s / q_s) is then the same double
# for s = 0 and s = 1 at every pick: the lowest s must win every time.  On exact fixtures, so bit for bit.
SCALE_TIE = dict(scales=(0.0, 1.0), bias=(1.0, 1.0))


def scale_tie_reference(f, trace=None):
    psf, res = np.array(exact_psf(f.N)), residual_of(f)
    model = np.zeros_like(res)
    stats = msclean_ref.msclean(psf, res, model, list(SCALE_TIE["scales"]), list(SCALE_TIE["bias"]), f.gain, 0.0, f.niter,
                                f.border, f.patch, trace=trace)
    return model, res, stats


def scale_tie_fixtures():
    names = ("d-rows-4-1-patch-N257", "e-later-entry-lower-index-N300", "g-sign-of-the-lower-N130", "rim-N17-patch1-border0")
    return [f for f in tie_fixtures() + rim_fixtures() if f.name in names]
