"""A numpy restatement of include/gridhip.h, "direction-dependent calibration": the classes, the multi-direction StEFCal
iteration with an explicit LDL^H and the pivot rule, the rotation per direction, the stats and the subtraction of
directions.  It is the reference the GPU tests compare with, and tests/test_ddcal_host.py checks it on worked cases.

ddcal also returns the smallest pivot ratio d_j / H[j,j] it saw (over every iteration, cell and pivot up to and including
the first that fails; a pivot with H[j,j] = 0 counts as exactly 0; inf when nothing was iterated), and `pivots` receives
every one of them, so that a test can assert that its input sits far from the 1e-12 threshold - or on the other side of
it, for the cells meant to be unsolved - and never rides on it."""
import numpy as np

from gaincal_ref import _stream, classes

PIVOT = 1e-12


def model_sum(g, p, q, t, M):
    """sum_d g[d,t,p] M[d] conj(g[d,t,q])"""
    return (g[:, t, p] * M * np.conj(g[:, t, q])).sum(axis=0)


def chi2(g, p, q, t, V, M, s):
    r = V - model_sum(g, p, q, t, M)
    return float((s * (r.real ** 2 + r.imag ** 2)).sum())


def normal_equations(g, p, q, t, V, M, s, T, A):
    """-> H [T][A][D][D] (full Hermitian), b [T][A][D] of one iteration"""
    D = M.shape[0]
    H, b = np.zeros((T * A, D, D), dtype=np.complex128), np.zeros((T * A, D), dtype=np.complex128)

    def add(cell, x):  # the sum of x per cell (bincount: np.add.at takes seconds on a few million visibilities)
        return np.bincount(cell, weights=x.real, minlength=T * A) + 1j * np.bincount(cell, weights=x.imag, minlength=T * A)
    zp, zq = M * np.conj(g[:, t, q]), np.conj(M) * np.conj(g[:, t, p])  # [D][n]
    for z, a, y in ((zp, p, V), (zq, q, np.conj(V))):
        cell = t * A + a
        for d in range(D):
            b[:, d] += add(cell, s * np.conj(z[d]) * y)
            for e in range(D):
                H[:, d, e] += add(cell, s * np.conj(z[d]) * z[e])
    H, b = H.reshape(T, A, D, D), b.reshape(T, A, D)
    return H, b


def ldl_solve(H, b):
    """H g = b by LDL^H without pivoting, in direction order.  -> (g or None when a pivot fails, the pivot ratios seen)"""
    D = len(b)
    L, d, ratios, ok = np.eye(D, dtype=np.complex128), np.zeros(D), [], True
    with np.errstate(all="ignore"):
        for j in range(D):
            hjj = H[j, j].real
            d[j] = hjj - (np.abs(L[j, :j]) ** 2 * d[:j]).sum()
            ratios.append(d[j] / hjj if hjj > 0 else 0.0)  # (an empty row - no data, a zero model - counts as exactly 0)
            if not d[j] > PIVOT * hjj:
                ok = False  # (the pivots after a failed one mean nothing and are not recorded)
                break
            for i in range(j + 1, D):
                L[i, j] = (H[i, j] - (L[i, :j] * np.conj(L[j, :j]) * d[:j]).sum()) / d[j]
    if not ok:
        return None, ratios
    y = np.zeros(D, dtype=np.complex128)
    for i in range(D):
        y[i] = b[i] - (L[i, :i] * y[:i]).sum()
    y /= d
    x = np.zeros(D, dtype=np.complex128)
    for i in range(D - 1, -1, -1):
        x[i] = y[i] - (np.conj(L[i + 1:, i]) * x[i + 1:]).sum()
    return x, ratios


def ddcal(vis, model_vis, a1, a2, A, slot=None, T=1, wt=None, mode=0, refant=0, gains=None, niter=50, tol=1e-8,
          history=None, pivots=None):
    """-> (gains [D][T][A], stats[8], the smallest pivot ratio); model_vis is [D][n]; gains given: the warm start (not
    modified).  history: a list that receives rel of every iteration; pivots: one that receives every pivot ratio."""
    V = np.asarray(vis, dtype=np.complex128)
    M = np.asarray(model_vis, dtype=np.complex128)
    n = V.shape[0]
    M = M.reshape(-1, n) if n else M.reshape(M.shape[0] if M.ndim == 2 else 1, 0)
    D = M.shape[0]
    a1, a2, slot, wt = _stream(n, a1, a2, slot, wt)
    used, flagged, dropped = classes(a1, a2, slot, wt, A, T)
    p, q, t, s = a1[used], a2[used], slot[used], wt[used]
    V, M = V[used], M[:, used]
    one = np.ones((D, T, A), dtype=np.complex128)
    g = one.copy() if gains is None else np.array(gains, dtype=np.complex128).reshape(D, T, A)
    ever = np.zeros((T, A), dtype=bool)
    chi0 = chi2(one, p, q, t, V, M, s)
    iters, rel, worst = 0, np.nan, np.inf
    for i in range(niter):
        H, b = normal_equations(g, p, q, t, V, M, s, T, A)
        gn = g.copy()
        for ti in range(T):
            for a in range(A):
                x, ratios = ldl_solve(H[ti, a], b[ti, a])
                worst = min([worst] + ratios)
                if pivots is not None:
                    pivots.extend(ratios)
                if x is None:
                    continue  # UNSOLVED in this iteration: all D gains keep their bits
                ever[ti, a] = True
                if mode == 1:
                    mag = np.abs(x)
                    x = np.where(mag > 0, x / np.where(mag > 0, mag, 1.0), g[:, ti, a])
                if i % 2 == 1:
                    x = (x + g[:, ti, a]) / 2
                gn[:, ti, a] = x
        rel = float(np.sqrt((np.abs(gn - g) ** 2).sum() / (np.abs(gn) ** 2).sum()))
        g, iters = gn, i + 1
        if history is not None:
            history.append(rel)
        if tol > 0 and rel <= tol:
            break
    if refant >= 0:
        for d in range(D):
            for ti in range(T):
                r = g[d, ti, refant]
                if ever[ti, refant] and np.abs(r) > 0 and np.isfinite(np.abs(r)):
                    g[d, ti] = np.where(ever[ti], g[d, ti] * (np.conj(r) / np.abs(r)), g[d, ti])
                    g[d, ti, refant] = np.abs(r)
    stats = np.array([iters, rel, chi2(g, p, q, t, V, M, s), chi0, used.sum(), flagged.sum(), dropped.sum(),
                      (~ever).sum()], dtype=np.float64)
    return g, stats, worst


def dd_subtract(gains, model_vis, a1, a2, slot=None, directions=None, vis=None):
    """-> vis - sum over the chosen directions (ascending) of g[d,t,p] M[d] conj(g[d,t,q]); vis None: + the sum"""
    g = np.asarray(gains, dtype=np.complex128)
    D, T, A = g.shape
    M = np.asarray(model_vis, dtype=np.complex128).reshape(D, -1)
    n = M.shape[1]
    a1, a2, slot, _ = _stream(n, a1, a2, slot, None)
    dirs = range(D) if directions is None else sorted(directions)
    inrange = (a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (slot >= 0) & (slot < T)
    p, q, t = np.where(inrange, a1, 0), np.where(inrange, a2, 0), np.where(inrange, slot, 0)
    out = np.zeros(n, dtype=np.complex128) if vis is None else np.array(vis, dtype=np.complex128)
    sign = 1.0 if vis is None else -1.0
    for d in dirs:
        term = (g[d, t, p] * M[d]) * np.conj(g[d, t, q])
        out = np.where(inrange, out + sign * term, out)
    return out
