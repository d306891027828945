"""A numpy restatement of the imaging weights (include/gridhip.h, "imaging weights"), written from the rules and not from
the library, which it does not import: what tests/test_gpu_weights.py compares the device with.

    flagged   s_k not > 0 (zero, negative, NaN): w_k = +0.0, and the visibility takes part in nothing else
    c_k       doweight's cell of (u_k / lam, v_k / lam): x = N // 2 + p N, floor(x + 0.5) per axis; -1 outside the grid or NaN
    D[c]      sum of s_k over the unflagged visibilities of cell c
    t_k       exp(-(u_k^2 + v_k^2) / (2 sigma^2)), 1 for sigma = 0
    natural   w = s t ;  uniform  w = (s / D) t ;  briggs  w = s / (1 + D f^2) t,  f^2 = (5 * 10^-R)^2 / (sum D^2 / sum D)
    outside   an unflagged visibility with c_k = -1 keeps s t and is left out of D, f^2 and the sums
    stats     [sum w, sum w^2 / s, sum s, noise, f^2, n_used, n_flagged, n_outside]
"""
import math

import numpy as np

MODES = {"natural": 0, "uniform": 1, "briggs": 2}


def cells(N, lam, u, v):
    """the flat cell y * N + x of every visibility, -1 outside the grid or for NaN coordinates"""
    with np.errstate(invalid="ignore"):
        pu, pv = np.asarray(u, dtype=np.float64) / np.float64(lam), np.asarray(v, dtype=np.float64) / np.float64(lam)
        fx = np.floor((np.float64(N // 2) + pu * np.float64(N)) + 0.5)
        fy = np.floor((np.float64(N // 2) + pv * np.float64(N)) + 0.5)
        ok = np.isfinite(fx) & np.isfinite(fy) & (fx >= 0) & (fy >= 0) & (fx < N) & (fy < N) & ~np.isnan(pu) & ~np.isnan(pv)
    x = np.where(ok, fx, 0).astype(np.int64)
    y = np.where(ok, fy, 0).astype(np.int64)
    return np.where(ok, y * N + x, -1)


def weights(N, lam, u, v, mode, robust=0.0, sigma=0.0, s=None):
    """-> (w, stats, D): the weights, the 8 stats and the N * N density (integer counts when s is None)"""
    mode = MODES.get(mode, mode)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = len(u)
    counts = s is None
    s = np.ones(n) if counts else np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = s > 0
    c = cells(N, lam, u, v)
    inside = live & (c >= 0)
    if counts:
        D = np.bincount(c[inside], minlength=N * N).astype(np.int64)
        sd, sd2 = int(D.sum()), int((D * D).sum())
    else:
        D = np.zeros(N * N)
        np.add.at(D, c[inside], s[inside])
        sd, sd2 = float(D.sum()), float((D * D).sum())
    f2 = 0.0
    if mode == 2 and sd > 0:
        b = 5.0 * 10.0 ** (-float(robust))
        f2 = (b * b) / (float(sd2) / float(sd))
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.exp(-((u * u + v * v) / (2.0 * sigma * sigma))) if sigma > 0 else np.ones(n)
    w = np.zeros(n)
    out = live & (c < 0)
    w[out] = s[out] * t[out]
    Dk = D[np.where(inside, c, 0)].astype(np.float64)
    if mode == 0:
        w[inside] = (s * t)[inside]
    elif mode == 1:
        w[inside] = ((s[inside] / Dk[inside]) * t[inside])
    else:
        w[inside] = (s[inside] / (1.0 + Dk[inside] * f2)) * t[inside]
    wi, si = w[inside], s[inside]
    sw, sw2s, ss = math.fsum(wi), math.fsum(wi * wi / si), math.fsum(si)
    noise = math.sqrt(sw2s * ss) / sw if sw != 0 else float("nan")
    stats = np.array([sw, sw2s, ss, noise, f2, inside.sum(), (~live).sum(), out.sum()], dtype=np.float64)
    return w, stats, D
