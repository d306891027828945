"""Inputs that test_coord_cases_host.py (host) and test_gpu_coords.py (GPU) share: coordinates that sit exactly on, and
one, two and three doubles either side of, every cell boundary and every sub-cell boundary of an axis, classified by what a
wrong coordinate rule would do with them, and integer-valued tables that make every comparison exact.  No GPU and no
library: plain numpy.

The rule (src/Gridding.hs:126-140, restated here and not taken from oracle/): for an axis of n cells oversampled Q
times, with every operation rounded to a double on its own,

    x = n // 2 + p * n ;  cell = floor(x + 0.5 / Q) ;  d = (x - cell) * Q ;  sub-cell = clamp(round(d), 0, Q - 1)

where `round` is libm's (halves away from zero).  The classes of a candidate p:

    cell tie               x + 0.5 / Q (as computed) is an integer: p sits on the floor's step
    sub-cell tie           d has the fractional part 0.5 exactly: p sits on the round's step
    low / high clamp       round(d) is -1 / Q: only the clamp keeps the sub-cell inside the table
    rint-sensitive         rounding halves to even instead picks another sub-cell
    contraction-sensitive  x computed with one rounding, as a fused multiply-add does, picks another (cell, sub-cell)

`grid` and the simple predictor use another rule, floor(0.5 + H * p) with H for both axes (src/Gridding.hs:95-112)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

GRIDS = ((49, 33), (64, 64), (100, 257))           # (H, Wd): odd, power of two, even and non-square
AXES = (33, 49, 64, 100, 257)                      # the axis sizes those grids have
QS = (1, 2, 3, 4, 5, 8)
SUPPORTS = ((1, 1), (5, 5), (7, 7), (17, 17), (9, 5))   # (gh, gw): 17 x 17 in parts of the tap list, 9 x 5 in sub-footprints
W = 2
VMAX = 3                                           # integer values in -VMAX .. VMAX, as sorted_cases.VMAX
HARD = ((49, 33, 3), (100, 257, 8))                # (H, Wd, Q) of the option matrix


def neighbours(p, k):
    """p and the k doubles on each side of it, for every element of p"""
    p = np.asarray(p, dtype=np.float64)
    out, lo, hi = [p], p, p
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def targets(n, Q):
    """every cell boundary and sub-cell boundary of the axis, in cells from the grid's centre, two cells past each edge"""
    j, r = np.arange(-2, n + 3, dtype=np.float64), np.arange(0, Q + 1, dtype=np.float64)
    return (j[:, None] - n // 2 + (r[None, :] - 0.5) / Q).ravel()


def candidates(n, Q, k=3):
    """sorted, distinct: p0 = t / n for every target t, and the k doubles on each side of p0.  (Three: with two, the
    49 x 33 grid at Q = 1 has 28 contraction-sensitive candidates on its two axes, with three it has 34.)"""
    return np.unique(neighbours(targets(n, Q) / n, k))


def libm_round(d):
    """halves away from zero, by truncation and a compare of the (exact) fractional part"""
    t = np.trunc(d)
    return t + np.where(np.abs(d - t) >= 0.5, np.copysign(1.0, d), 0.0)


def rule_from_x(x, Q, rnd=libm_round):
    """(cell, unclamped sub-cell, d, x + 0.5 / Q) of x = n // 2 + p * n, all as doubles"""
    s = x + 0.5 / np.float64(Q)
    cell = np.floor(s)
    d = (x - cell) * np.float64(Q)
    return cell, rnd(d), d, s


def rule(n, Q, p, rnd=libm_round):
    """(cell, sub-cell) as int64 for finite, moderate p"""
    x = np.float64(n // 2) + np.asarray(p, dtype=np.float64) * np.float64(n)
    cell, r, _, _ = rule_from_x(x, Q, rnd)
    return cell.astype(np.int64), np.clip(r, 0, Q - 1).astype(np.int64)


def fused_x(n, p):
    """n // 2 + p * n rounded once: what a fused multiply-add gives (exact rationals, then the nearest double)"""
    return np.array([float(Fraction(float(q)) * n + n // 2) for q in p], dtype=np.float64)


Classes = namedtuple("Classes", "cell_tie sub_tie low_clamp high_clamp rint contraction")


def classify(n, Q, p):
    """boolean masks over p, one per class of the module docstring"""
    p = np.asarray(p, dtype=np.float64)
    x = np.float64(n // 2) + p * np.float64(n)
    cell, r, d, s = rule_from_x(x, Q)
    sub = np.clip(r, 0, Q - 1)
    _, r_even, _, _ = rule_from_x(x, Q, np.rint)
    cell_f, r_f, _, _ = rule_from_x(fused_x(n, p), Q)
    return Classes(cell_tie=s == np.floor(s), sub_tie=np.abs(d - np.trunc(d)) == 0.5, low_clamp=r == -1, high_clamp=r >= Q,
                   rint=np.clip(r_even, 0, Q - 1) != sub, contraction=(cell_f != cell) | (np.clip(r_f, 0, Q - 1) != sub))


def ulp_pairs(n, Q):
    """(p, p') one double apart with different sub-cells or cells: the pairs among the candidates that straddle a step"""
    c = candidates(n, Q)
    a, b = c[:-1], c[1:]
    adj = np.nextafter(a, np.inf) == b
    ca, fa = rule(n, Q, a)
    cb, fb = rule(n, Q, b)
    m = adj & ((ca != cb) | (fa != fb))
    return a[m], b[m]


def wavelengths(p, lam):
    """coordinates in wavelengths for the callers that divide by lam themselves: p * lam and the double on each side of
    it, so that u / lam (what the device computes, and what the classes are then counted on) lands on and next to p"""
    return np.unique(neighbours(np.asarray(p, dtype=np.float64) * np.float64(lam), 1))


# ---- the `grid` rule -------------------------------------------------------------------------------------------------
def grid_rule(H, p):
    """floor(0.5 + H * p) as a double (the cell is H // 2 + that, on both axes)"""
    return np.floor(0.5 + np.float64(H) * np.asarray(p, dtype=np.float64))


def grid_candidates(H, n):
    """for an axis of n cells binned with H: H * p = j - 0.5 and its two neighbours each side, two cells past each edge,
    and H * p = 0.49999999999999994 (where 0.5 + H * p rounds up to 1)"""
    j = np.arange(-2, n + 3, dtype=np.float64) - H // 2
    return np.unique(np.concatenate([neighbours((j - 0.5) / H, 2), neighbours([0.49999999999999994 / H], 2)]))


# ---- extremes --------------------------------------------------------------------------------------------------------
def extremes(n, S):
    """zeros and denormals, the first and last cells whose footprint (support S) still touches an axis of n cells, the
    doubles either side of 2^31 / n and 2^63 / n, and +-1e300, +-inf, NaN"""
    k = np.arange(S // 2 - 2, S // 2 + 4, dtype=np.float64)
    edge = 0.5 + k / n
    big = neighbours([2.0 ** 31 / n, 2.0 ** 63 / n], 1)
    pos = np.concatenate([[0.0, 5e-324], edge, big, [1e300, np.inf]])
    return np.concatenate([pos, -pos, [np.nan]])


def touches(n, S, cell):
    """the footprint of support S centred by the reference's rule on `cell` (a double, may be huge or non-finite) has a
    tap inside the axis"""
    with np.errstate(invalid="ignore"):
        x0 = cell - S // 2
        return np.isfinite(cell) & (x0 > -S) & (x0 < n)


# ---- integer data ----------------------------------------------------------------------------------------------------
_MARK = np.array([-3, -2, -1, 1, 2, 3, -1, 2])      # no zero, neighbours differ, and so do the last and the first


def cint(rng, shape):
    return (rng.integers(-VMAX, VMAX + 1, shape) + 1j * rng.integers(-VMAX, VMAX + 1, shape)).astype(np.complex128)


def int_gcf(Q, gh, gw, seed=0):
    """[W, Q, Q, gh, gw] integer taps; tap (0, 0) of slice (w, yf, xf) is marked with (xf, yf, w), so that any two slices
    next to each other on an axis differ, whatever the random taps are"""
    rng = np.random.default_rng(100 * gh + 10 * gw + Q + seed)
    g = cint(rng, (W, Q, Q, gh, gw))
    q = np.arange(Q)
    sign = np.array([1.0, -1.0])
    g[:, :, :, 0, 0] = _MARK[q][None, None, :] + 1j * sign[:, None, None] * _MARK[q][None, :, None]
    return g


def int_grid(H, Wd, seed=0):
    return cint(np.random.default_rng(7 * H + Wd + seed), (H, Wd))


Stream = namedtuple("Stream", "H Wd Q u v wb vis keep nbad")


def tie_stream(H, Wd, Q, extra_u=(), extra_v=(), seed=0):
    """A permutation of the u-candidates (and extra_u) paired with the v-candidates (and extra_v), the shorter list
    repeated; integer visibilities; w-planes 0 .. W - 1, except that every 37th visibility whose cell is inside the
    grid on both axes takes the plane W or -1: it must be left out and counted (`nbad` of them; keep = the others)."""
    rng = np.random.default_rng(1000 * H + 10 * Wd + Q + seed)
    cu = np.concatenate([candidates(Wd, Q), np.asarray(extra_u, dtype=np.float64)])
    cv = np.concatenate([candidates(H, Q), np.asarray(extra_v, dtype=np.float64)])
    n = max(len(cu), len(cv))
    u, v = rng.permutation(np.resize(cu, n)), np.resize(cv, n)
    wb = rng.integers(0, W, n)
    x, _ = rule(Wd, Q, u)
    y, _ = rule(H, Q, v)
    inside = np.flatnonzero((x >= 0) & (x < Wd) & (y >= 0) & (y < H))[::37]
    wb[inside[0::2]] = W
    wb[inside[1::2]] = -1
    keep = (wb >= 0) & (wb < W)
    return Stream(H, Wd, Q, u, v, wb.astype(np.int64), cint(rng, n), keep, len(inside))


def sum_bound(n, gh, gw):
    """no partial sum of n visibilities' products with gh x gw taps, in any order, exceeds this: each part of a product
    of two complex integers with parts in -VMAX .. VMAX is at most 2 VMAX^2"""
    return n * gh * gw * 2 * VMAX * VMAX
