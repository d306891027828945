"""A numpy restatement of residual flagging (include/gridhip.h, "residual flagging") that sorts: what the GPU tests compare
with, bit for bit.  Every step is the header's: the classes in their order, the amplitude as np.sqrt(re * re + im * im)
(never np.abs, which is hypot), the lower median as the element of rank (n - 1) // 2 of a sort, the MAD likewise over
|a - med|, T = med + nsigma * (1.4826 * MAD) with each operation rounded once."""
import numpy as np

KEPT, FLAGGED, LEFT, NOT_FINITE, ABOVE_AMAX, CLIPPED = 0, 1, 2, 3, 4, 16


def amplitude(vis, model_vis=None):
    vis = np.asarray(vis, dtype=np.complex128)
    re, im = vis.real.copy(), vis.imag.copy()
    if model_vis is not None:
        m = np.asarray(model_vis, dtype=np.complex128)
        re, im = re - m.real, im - m.imag
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im)


def lower_median(x):
    return np.sort(x)[(len(x) - 1) // 2]


def group_round(a, nsigma, min_count):
    """{ n, med, MAD, T } of one group's participants"""
    n = len(a)
    if n == 0:
        return 0.0, np.nan, np.nan, np.inf
    med = lower_median(a)
    mad = lower_median(np.abs(a - med))
    sigma = np.float64(1.4826) * mad
    T = np.inf if (n < min_count or sigma == 0.0) else med + np.float64(nsigma) * sigma
    return float(n), med, mad, T


def flag_residuals(vis, model_vis=None, group=None, G=1, weights=None, nsigma=5.0, amax=0.0, min_count=8, niter=3):
    """-> (wt_out, flags, group_stats, stats) as gridhip_flag_residuals leaves them"""
    a = amplitude(vis, model_vis)
    n = len(a)
    s = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    g = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    flags = np.zeros(n, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        flagged = ~(s > 0.0)
    left = ~flagged & ((g < 0) | (g >= G))
    tested = ~flagged & ~left
    bad = tested & ~np.isfinite(a)
    high = tested & ~bad & (a > amax) if amax > 0.0 else np.zeros(n, dtype=bool)
    flags[flagged], flags[left], flags[bad], flags[high] = FLAGGED, LEFT, NOT_FINITE, ABOVE_AMAX
    part = flags == KEPT
    start = int(part.sum())
    gstats = np.empty((G, 4))
    gstats[:] = (0.0, np.nan, np.nan, np.inf)
    if niter == 0:
        gstats[:, 0] = np.bincount(g[part], minlength=G)
    rounds = clipped = 0
    for r in range(niter):
        rounds += 1
        gstats[:] = (0.0, np.nan, np.nan, np.inf)
        idx = np.flatnonzero(part)
        order = idx[np.argsort(g[idx], kind="stable")]
        bounds = np.flatnonzero(np.diff(g[order])) + 1
        clip = []
        for members in np.split(order, bounds) if len(order) else []:
            gg = g[members[0]]
            gstats[gg] = group_round(a[members], nsigma, min_count)
            clip.append(members[a[members] > gstats[gg, 3]])
        clip = np.concatenate(clip) if clip else np.zeros(0, dtype=np.int64)
        flags[clip] = CLIPPED + r
        part[clip] = False
        clipped += len(clip)
        if len(clip) == 0:
            break
    wt_out = np.where((flags == KEPT) | (flags == LEFT), s, 0.0)
    stats = np.array([rounds, start, clipped, bad.sum(), high.sum(), left.sum(), flagged.sum(), start - clipped],
                     dtype=np.float64)
    return wt_out, flags, gstats, stats


def same_bits(x, y):
    """equal as bit patterns (NaN in the same places, +0.0 distinct from -0.0), the same shape and dtype"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
