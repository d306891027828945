"""A numpy restatement of include/gridhip.h, "gain calibration": the StEFCal iteration with solution intervals, the
reference-antenna rotation, the stats, and the application of gains.  It is the reference the GPU tests compare with,
and tests/test_gaincal_host.py checks it on cases worked by hand."""
import numpy as np


def classes(a1, a2, slot, wt, A, T):
    """-> (used, flagged, dropped) boolean masks: flagged is looked at first, autocorrelations count as dropped"""
    flagged = ~(wt > 0)  # (zero, negative and NaN alike)
    inrange = (a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (slot >= 0) & (slot < T)
    dropped = ~flagged & (~inrange | (a1 == a2))
    return ~flagged & ~dropped, flagged, dropped


def _stream(n, a1, a2, slot, wt):
    a1, a2 = np.asarray(a1, dtype=np.int64), np.asarray(a2, dtype=np.int64)
    slot = np.zeros(n, dtype=np.int64) if slot is None else np.asarray(slot, dtype=np.int64)
    wt = np.ones(n) if wt is None else np.asarray(wt, dtype=np.float64)
    return a1, a2, slot, wt


def chi2(g, p, q, t, V, M, s):
    r = V - g[t, p] * M * np.conj(g[t, q])
    return float((s * (r.real ** 2 + r.imag ** 2)).sum())


def gaincal(vis, model_vis, a1, a2, A, slot=None, T=1, wt=None, mode=0, refant=0, gains=None, niter=50, tol=1e-8,
            history=None):
    """-> (gains [T][A], stats[8]); gains given: the warm start (not modified).  history: a list that receives rel
    of every iteration."""
    V, M = np.asarray(vis, dtype=np.complex128), np.asarray(model_vis, dtype=np.complex128)
    n = V.shape[0]
    a1, a2, slot, wt = _stream(n, a1, a2, slot, wt)
    used, flagged, dropped = classes(a1, a2, slot, wt, A, T)
    p, q, t, s = a1[used], a2[used], slot[used], wt[used]
    V, M = V[used], M[used]
    X, Y = (s * V) * np.conj(M), s * (M.real ** 2 + M.imag ** 2)
    g = np.ones((T, A), dtype=np.complex128) if gains is None else np.array(gains, dtype=np.complex128).reshape(T, A)
    ever = np.zeros((T, A), dtype=bool)
    chi0 = chi2(np.ones((T, A), dtype=np.complex128), p, q, t, V, M, s)
    iters, rel = 0, np.nan
    for i in range(niter):
        num, den = np.zeros((T, A), dtype=np.complex128), np.zeros((T, A))
        np.add.at(num, (t, p), X * g[t, q])
        np.add.at(den, (t, p), Y * np.abs(g[t, q]) ** 2)
        np.add.at(num, (t, q), np.conj(X) * g[t, p])
        np.add.at(den, (t, q), Y * np.abs(g[t, p]) ** 2)
        ok = den > 0
        ever |= ok
        gn = np.where(ok, num / np.where(ok, den, 1.0), g)
        if mode == 1:
            mag = np.abs(gn)
            gn = np.where(ok, np.where(mag > 0, gn / np.where(mag > 0, mag, 1.0), g), g)
        if i % 2 == 1:
            gn = np.where(ok, (gn + g) / 2, g)
        rel = float(np.sqrt((np.abs(gn - g) ** 2).sum() / (np.abs(gn) ** 2).sum()))
        g, iters = gn, i + 1
        if history is not None:
            history.append(rel)
        if tol > 0 and rel <= tol:
            break
    if refant >= 0:
        for ti in range(T):
            r = g[ti, refant]
            if ever[ti, refant] and np.abs(r) > 0 and np.isfinite(np.abs(r)):
                g[ti] = np.where(ever[ti], g[ti] * (np.conj(r) / np.abs(r)), g[ti])  # (an unsolved gain keeps its bits)
                g[ti, refant] = np.abs(r)
    stats = np.array([iters, rel, chi2(g, p, q, t, V, M, s), chi0, used.sum(), flagged.sum(), dropped.sum(),
                      (~ever).sum()], dtype=np.float64)
    return g, stats


def apply_gains(gains, vis, a1, a2, slot=None, wt=None, inverse=True):
    """-> (vis_out, wt_out)"""
    g = np.asarray(gains, dtype=np.complex128)
    T, A = g.shape
    V = np.asarray(vis, dtype=np.complex128)
    n = V.shape[0]
    a1, a2, slot, wt = _stream(n, a1, a2, slot, wt)
    inrange = (a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (slot >= 0) & (slot < T)
    p, q, t = np.where(inrange, a1, 0), np.where(inrange, a2, 0), np.where(inrange, slot, 0)
    gp, gq = g[t, p], g[t, q]
    out, wout = V.copy(), wt.copy()
    if not inverse:
        out[inrange] = (gp * V * np.conj(gq))[inrange]
        return out, wout
    with np.errstate(all="ignore"):
        n2p, n2q = gp.real ** 2 + gp.imag ** 2, gq.real ** 2 + gq.imag ** 2
        good = inrange & (n2p > 0) & (n2q > 0) & np.isfinite(n2p) & np.isfinite(n2q)
        d = np.where(good, gp * np.conj(gq), 1.0)
        out = np.where(good, V / d, V)
        wout = np.where(good, wt * n2p * n2q, 0.0)
    return out, wout
