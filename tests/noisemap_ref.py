"""Local background and noise maps restated in numpy, statement by statement as include/gridhip.h ("local background and
noise maps") defines them: the reference the noise_map tests compare the library with, bit for bit.  The node statistic is
a sort of image_stats' keys (tests/noise_ref.py) inside plain loops over the nodes and the clip rounds.  The maps are
evaluated a whole image at a time, every operation of a lerp one numpy call - a difference, a product, a sum, each rounded
once, nothing fused - and interp_cell says the same for one cell in plain Python, for the hand-computed checks."""
import math

import numpy as np

import noise_ref

MODES = {None: 0, "subtract": 1, "snr": 2}


def centres(N, border, step):
    """the node centres c_i, the same along y and x"""
    M = N - 2 * border
    G = max(1, M // step)
    return [border + min(i * step + step // 2, M - 1) for i in range(G)]


def takes_part(image, mask, exclude, border):
    N = image.shape[0]
    take = np.zeros((N, N), dtype=bool)
    take[border:N - border, border:N - border] = True
    take &= np.isfinite(image)
    if mask is not None:
        take &= (np.asarray(mask) == 0) if exclude else (np.asarray(mask) != 0)
    return take


def node_stat(v, kappa, nclip):
    """(med, MAD, n_used, rounds) of the 1-d float64 array v of one window's cells that take part"""
    r = 0
    med = mad = math.nan
    while v.size:
        med = noise_ref.lower_median(v)
        with np.errstate(over="ignore"):
            d = np.abs(v - med)  # (rounded once; it may overflow to +Inf, which still has its key)
        mad = noise_ref.lower_median(d)
        if r == nclip:
            break
        L = kappa * (1.4826 * mad)
        keep = ~(d > L)
        if keep.all():
            break
        v = v[keep]
        r += 1
    return med, mad, int(v.size), r


def node_table(image, mask=None, exclude=False, border=0, step=16, half=32, kappa=3.0, nclip=3, min_count=16):
    """nodes[4][G][G] = background, rms, n_used, rounds"""
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    take = takes_part(image, mask, exclude, border)
    c = centres(N, border, step)
    G = len(c)
    nodes = np.empty((4, G, G))
    lo, hi = border, N - border  # the window is clipped to the border region
    for i in range(G):
        y0, y1 = max(c[i] - half, lo), min(c[i] + half + 1, hi)
        for j in range(G):
            x0, x1 = max(c[j] - half, lo), min(c[j] + half + 1, hi)
            win = image[y0:y1, x0:x1]
            med, mad, n, r = node_stat(win[take[y0:y1, x0:x1]], kappa, nclip)
            enough = n >= min_count
            nodes[0, i, j] = med if enough else math.nan
            nodes[1, i, j] = 1.4826 * mad if enough and mad > 0 else math.nan
            nodes[2, i, j] = n
            nodes[3, i, j] = r
    return nodes


def locate(p, c):
    """(i, i1, f) of the coordinate p among the centres c"""
    i = 0
    for q in range(len(c)):  # the largest node with c_i <= p, or 0
        if c[q] <= p:
            i = q
    i1 = min(i + 1, len(c) - 1)
    f = 0.0 if i1 == i or p < c[i] else float(p - c[i]) / float(c[i1] - c[i])
    return i, i1, f


def lerp(a, b, f):
    """one cell, in plain Python: each operation rounded once"""
    fa, fb = math.isfinite(a), math.isfinite(b)
    if fa and fb:
        d = b - a
        p = f * d
        return a + p
    return a if fa else b if fb else math.nan


def interp_cell(table, c, y, x):
    i, i1, fy = locate(y, c)
    j, j1, fx = locate(x, c)
    t = [[float(table[a, b]) for b in (j, j1)] for a in (i, i1)]
    return lerp(lerp(t[0][0], t[0][1], fx), lerp(t[1][0], t[1][1], fx), fy)


def lerp_all(a, b, f, branches=None):
    """lerp over arrays; branches, when given, counts the cells that took [both, only a, only b, neither]"""
    fa, fb = np.isfinite(a), np.isfinite(b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        p = f * d
        both = a + p
    if branches is not None:
        for q, m in enumerate((fa & fb, fa & ~fb, ~fa & fb, ~fa & ~fb)):
            branches[q] += int(np.count_nonzero(m))
    return np.where(fa & fb, both, np.where(fa, a, np.where(fb, b, np.nan)))


def interp_map(table, N, border, step, branches=None):
    """the N x N map of a G x G table: NaN outside the border region"""
    c = centres(N, border, step)
    loc = [locate(p, c) for p in range(border, N - border)]
    i = np.array([l[0] for l in loc])
    i1 = np.array([l[1] for l in loc])
    f = np.array([l[2] for l in loc], dtype=np.float64)
    fx, fy = f[None, :], f[:, None]
    top = lerp_all(table[i][:, i], table[i][:, i1], fx, branches)
    bot = lerp_all(table[i1][:, i], table[i1][:, i1], fx, branches)
    out = np.full((N, N), np.nan)
    out[border:N - border, border:N - border] = lerp_all(top, bot, fy, branches)
    return out


def noise_map(image, mask=None, exclude=False, border=0, step=16, half=None, kappa=3.0, nclip=3, min_count=16, mode=None,
              branches=None):
    """(background, rms, out, nodes, stats) as Context.noise_map returns them (out is None for mode None).  branches: a
    list of 4 zeros that receives the lerp branches the RMS map took, see lerp_all."""
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    half = min(64, 2 * step) if half is None else half
    nodes = node_table(image, mask, exclude, border, step, half, kappa, nclip, min_count)
    G = nodes.shape[1]
    bg = interp_map(nodes[0], N, border, step)
    rms = interp_map(nodes[1], N, border, step, branches)
    m = MODES[mode]
    out, bad = None, 0
    if m:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out = image - bg
            if m == 2:
                out = out / rms
        inner = out[border:N - border, border:N - border]
        bad = int(np.count_nonzero(~np.isfinite(inner)))
    have = nodes[1][~np.isnan(nodes[1])]
    if have.size:
        k = np.sort(noise_ref.keys(have))
        lo, hi = (float(v) for v in noise_ref.values(k[[0, -1]]))
    else:
        lo = hi = math.nan
    stats = np.array([float(G), float(np.count_nonzero(~np.isnan(nodes[0]))), float(have.size), lo, hi, float(bad),
                      float(nodes[3].max()), 0.0])
    return bg, rms, out, nodes, stats
