"""A numpy restatement of include/gridhip.h, "polarisation": the matrix StEFCal iteration with solution intervals, the
common-phase rotation, the stats, the application of Jones matrices and the change between correlations and Stokes
parameters.  Written from the header text with explicit 2x2 products in the stated order; it is the reference the GPU
tests compare with, and tests/test_jonescal_host.py checks it on cases worked by hand.

A stack of 2x2 matrices is an array [..., 2, 2] complex128."""
import numpy as np

from gaincal_ref import _stream, classes


def cx(re, im):
    """re + im i with the very bits of both (re + 1j * im would lose a zero's sign and turn an Inf into a NaN)"""
    z = np.empty(np.broadcast(re, im).shape, dtype=np.complex128)
    z.real, z.imag = re, im
    return z


def cmul(a, b):
    """(a c - b d) + (a d + b c) i, every product and sum rounded on its own (numpy's own complex product is not relied on)"""
    return cx(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


def mm(X, Y):
    """C[i][j] = X[i][0] Y[0][j] + X[i][1] Y[1][j]"""
    X, Y = np.broadcast_arrays(X, Y)
    C = np.empty(X.shape, dtype=np.complex128)
    for i in (0, 1):
        for j in (0, 1):
            C[..., i, j] = cmul(X[..., i, 0], Y[..., 0, j]) + cmul(X[..., i, 1], Y[..., 1, j])
    return C


def herm(X):
    return np.conj(np.swapaxes(X, -1, -2))


def abs2(x):
    return x.real * x.real + x.imag * x.imag


def fro2(X):
    """((|x00|^2 + |x01|^2) + |x10|^2) + |x11|^2"""
    return ((abs2(X[..., 0, 0]) + abs2(X[..., 0, 1])) + abs2(X[..., 1, 0])) + abs2(X[..., 1, 1])


def chi2(G, p, q, t, V, M, s):
    return float((s * fro2(V - mm(mm(G[t, p], M), herm(G[t, q])))).sum())


def _side(num, den, t, a, Y, Mx, Gh, s):
    """one side of every used visibility into the sums of antenna a: Z = Mx Gh, sZ = s Z, num += Y (sZ)^H, den += Z (sZ)^H"""
    Z = mm(Mx, Gh)
    sZh = herm(s[:, None, None] * Z)
    N, D = mm(Y, sZh), mm(Z, sZh)
    np.add.at(num, (t, a), N)
    np.add.at(den, (t, a, 0), D[:, 0, 0].real)
    np.add.at(den, (t, a, 1), D[:, 1, 1].real)
    np.add.at(den, (t, a, 2), D[:, 0, 1].real)
    np.add.at(den, (t, a, 3), D[:, 0, 1].imag)


def jonescal(vis, model_vis, a1, a2, A, slot=None, T=1, wt=None, mode=0, refant=0, gains=None, niter=50, tol=1e-8,
             history=None):
    """-> (gains [T][A][2][2], stats[8]); gains given: the warm start (not modified).  history: a list that receives
    rel of every iteration."""
    V = np.asarray(vis, dtype=np.complex128).reshape(-1, 2, 2)
    M = np.asarray(model_vis, dtype=np.complex128).reshape(-1, 2, 2)
    n = V.shape[0]
    a1, a2, slot, wt = _stream(n, a1, a2, slot, wt)
    used, flagged, dropped = classes(a1, a2, slot, wt, A, T)
    p, q, t, s = a1[used], a2[used], slot[used], wt[used]
    V, M = V[used], M[used]
    eye = np.zeros((T, A, 2, 2), dtype=np.complex128)
    eye[..., 0, 0] = eye[..., 1, 1] = 1.0
    G = eye.copy() if gains is None else np.array(gains, dtype=np.complex128).reshape(T, A, 2, 2)
    if mode != 0:
        G[..., 0, 1] = G[..., 1, 0] = 0.0
    ever = np.zeros((T, A), dtype=bool)
    chi0 = float((s * fro2(V - M)).sum())
    iters, rel = 0, np.nan
    for i in range(niter):
        num, den = np.zeros((T, A, 2, 2), dtype=np.complex128), np.zeros((T, A, 4))  # d00, d11, re d01, im d01
        _side(num, den, t, p, V, M, herm(G[t, q]), s)
        _side(num, den, t, q, herm(V), herm(M), herm(G[t, p]), s)
        d00, d11, d01 = den[..., 0], den[..., 1], cx(den[..., 2], den[..., 3])
        Gn = G.copy()
        with np.errstate(all="ignore"):
            ok = (d00 > 0) & (d11 > 0)
            if mode == 0:
                e = d11 - abs2(d01) / d00
                ok &= e > 1e-12 * d11
                c = cx(d01.real / d00, d01.imag / d00)
                for r in (0, 1):
                    n0, n1 = num[..., r, 0], num[..., r, 1]
                    w = n1 - cmul(n0, c)
                    x1 = cx(w.real / e, w.imag / e)
                    x0 = cx(n0.real / d00, n0.imag / d00) - cmul(x1, np.conj(c))
                    Gn[..., r, 0], Gn[..., r, 1] = np.where(ok, x0, G[..., r, 0]), np.where(ok, x1, G[..., r, 1])
            else:
                for r, d in ((0, d00), (1, d11)):
                    x = cx(num[..., r, r].real / d, num[..., r, r].imag / d)
                    if mode == 2:
                        mag = np.sqrt(abs2(x))
                        x = np.where(mag > 0, cx(x.real / mag, x.imag / mag), G[..., r, r])
                    Gn[..., r, r] = np.where(ok, x, G[..., r, r])
        ever |= ok
        if i % 2 == 1:
            Gn = np.where(ok[..., None, None], (Gn + G) / 2, G)
        rel = float(np.sqrt(fro2(Gn - G).sum() / fro2(Gn).sum()))
        G, iters = Gn, i + 1
        if history is not None:
            history.append(rel)
        if tol > 0 and rel <= tol:
            break
    if refant >= 0:
        for ti in range(T):
            r = G[ti, refant, 0, 0]
            mag = np.sqrt(abs2(r))
            if ever[ti, refant] and mag > 0 and np.isfinite(mag):
                rot = cx(r.real / mag, -r.imag / mag)
                turned = cmul(G[ti], rot)
                if mode != 0:
                    turned[..., 0, 1] = turned[..., 1, 0] = 0.0
                G[ti] = np.where(ever[ti][:, None, None], turned, G[ti])  # (an unsolved gain keeps its bits)
                G[ti, refant, 0, 0] = mag
    stats = np.array([iters, rel, chi2(G, p, q, t, V, M, s), chi0, used.sum(), flagged.sum(), dropped.sum(),
                      (~ever).sum()], dtype=np.float64)
    return G, stats


def inverse(G):
    """-> (G^-1 = adj(G) conj(det) / |det|^2, |det|^2)"""
    det = cmul(G[..., 0, 0], G[..., 1, 1]) - cmul(G[..., 0, 1], G[..., 1, 0])
    nd = abs2(det)
    adj = np.empty(G.shape, dtype=np.complex128)
    adj[..., 0, 0], adj[..., 0, 1], adj[..., 1, 0], adj[..., 1, 1] = G[..., 1, 1], -G[..., 0, 1], -G[..., 1, 0], G[..., 0, 0]
    h = cmul(adj, np.conj(det)[..., None, None])
    return cx(h.real / nd[..., None, None], h.imag / nd[..., None, None]), nd


def apply_jones(gains, vis, a1, a2, slot=None, wt=None, inverse_=True):
    """-> (vis_out [n][2][2], wt_out)"""
    G = np.asarray(gains, dtype=np.complex128)
    T, A = G.shape[:2]
    V = np.asarray(vis, dtype=np.complex128).reshape(-1, 2, 2)
    n = V.shape[0]
    a1, a2, slot, wt = _stream(n, a1, a2, slot, wt)
    inrange = (a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (slot >= 0) & (slot < T)
    p, q, t = np.where(inrange, a1, 0), np.where(inrange, a2, 0), np.where(inrange, slot, 0)
    Gp, Gq = G[t, p], G[t, q]
    out, wout = V.copy(), wt.copy()
    with np.errstate(all="ignore"):
        if not inverse_:
            out[inrange] = mm(mm(Gp, V), herm(Gq))[inrange]
            return out, wout
        ip, np_ = inverse(Gp)
        iq, nq = inverse(Gq)
        good = inrange & (np_ > 0) & (nq > 0) & np.isfinite(np_) & np.isfinite(nq)
        out = np.where(good[:, None, None], mm(mm(ip, V), herm(iq)), V)
        wout = np.where(good, (wt * np.sqrt(np_)) * np.sqrt(nq), 0.0)
    return out, wout


ROWS = {0: (0, 1, 2, 3), 1: (0, 3, 1, 2)}  # basis -> the rows of (diagonal sum, diagonal difference, off sum, off difference)


def stokes(vis, basis=0, which=15, out=None):
    """[n][2][2] -> the [4][n] block I, Q, U, V; rows outside `which` keep what `out` held (zeros when None)"""
    V = np.asarray(vis, dtype=np.complex128).reshape(-1, 2, 2)
    a, b, c, d = V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1]
    S = np.zeros((4, V.shape[0]), dtype=np.complex128) if out is None else out.copy()
    rows = ROWS[basis]
    vals = (cx((a.real + d.real) / 2, (a.imag + d.imag) / 2), cx((a.real - d.real) / 2, (a.imag - d.imag) / 2),
            cx((b.real + c.real) / 2, (b.imag + c.imag) / 2), cx((b.imag - c.imag) / 2, (c.real - b.real) / 2))
    for r, v in zip(rows, vals):
        if which >> r & 1:
            S[r] = v
    return S


def stokes_inverse(S, basis=0):
    """the [4][n] block -> [n][2][2]"""
    S = np.asarray(S, dtype=np.complex128)
    x, y, u, w = (S[r] for r in ROWS[basis])
    V = np.empty((S.shape[1], 2, 2), dtype=np.complex128)
    V[:, 0, 0], V[:, 1, 1] = x + y, x - y
    V[:, 0, 1] = cx(u.real - w.imag, u.imag + w.real)
    V[:, 1, 0] = cx(u.real + w.imag, u.imag - w.real)
    return V
