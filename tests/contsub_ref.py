"""A numpy restatement of continuum subtraction (include/gridhip.h, "continuum subtraction"): what the GPU tests compare
with, bit for bit.  Every step is the header's: the Chebyshev table by the rounded recurrence, the classes in their order,
one accumulator chain per moment walked over the channels in ascending order, the normal matrix by the product identity,
LDL^T without pivoting with the fall-back at the first pivot that is not good, the clip rounds per row, and the closing
pass.  The rows are the vector axis: every numpy operation below is one rounded IEEE operation per row, in the order the
header fixes, so there is no tolerance to state."""
import numpy as np

USED, FLAGGED, MASKED, NOT_FINITE, CLIPPED = 0, 1, 2, 3, 16
PIVOT = 1e-12


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def canon(x):
    """NaN positions compared as positions: every NaN becomes the one NaN (real and imaginary parts on their own)"""
    x = np.array(x, order="C")
    parts = x.view(np.float64)
    parts[np.isnan(parts)] = np.nan
    return x


def chebyshev_table(x, degree):
    """T[p][c], p = 0 .. 2 degree: T_0 = 1, T_1 = x, T_{p+1} = (2 * x) * T_p - T_{p-1}, every operation rounded once"""
    x = np.asarray(x, dtype=np.float64)
    T = np.zeros((2 * degree + 1, x.size))
    T[0] = 1.0
    with np.errstate(all="ignore"):
        if degree >= 1:
            T[1] = x
        x2 = 2.0 * x
        for p in range(1, 2 * degree):
            T[p + 1] = x2 * T[p] - T[p - 1]
    return T


def _fit(part, w, vre, vim, T, D):
    """the moments of the participants and the solve: -> a_re, a_im [D + 1][R], degree [R], n [R]"""
    R, C = part.shape
    mu = [np.zeros(R) for _ in range(2 * D + 1)]
    bre = [np.zeros(R) for _ in range(D + 1)]
    bim = [np.zeros(R) for _ in range(D + 1)]
    with np.errstate(all="ignore"):
        for c in range(C):
            m, wc = part[:, c], w[:, c]
            if not m.any():
                continue
            for p in range(2 * D + 1):
                mu[p] = np.where(m, mu[p] + wc * T[p, c], mu[p])
            for k in range(D + 1):
                g = wc * T[k, c]
                bre[k] = np.where(m, bre[k] + g * vre[:, c], bre[k])
                bim[k] = np.where(m, bim[k] + g * vim[:, c], bim[k])
        n = part.sum(axis=1).astype(np.int64)
        A = [[0.5 * (mu[j + k] + mu[abs(j - k)]) for k in range(D + 1)] for j in range(D + 1)]
        L = [[np.zeros(R) for _ in range(D + 1)] for _ in range(D + 1)]
        d = [np.ones(R) for _ in range(D + 1)]
        deg = np.full(R, D, dtype=np.int64)
        opened = np.ones(R, dtype=bool)
        for k in range(D + 1):
            t = A[k][k]
            for p in range(k):
                t = t - (L[k][p] * L[k][p]) * d[p]
            good = opened & (A[k][k] > 0.0) & (t > PIVOT * A[k][k])
            deg = np.where(opened & ~good, k - 1, deg)
            opened = good
            d[k] = np.where(good, t, 1.0)
            for i in range(k + 1, D + 1):
                s = A[i][k]
                for p in range(k):
                    s = s - (L[i][p] * L[k][p]) * d[p]
                L[i][k] = np.where(good, s / d[k], 0.0)
        out = []
        for b in (bre, bim):
            z = [None] * (D + 1)
            for k in range(D + 1):
                s = b[k]
                for p in range(k):
                    s = s - L[k][p] * z[p]
                z[k] = s
            a = [None] * (D + 1)
            for k in range(D, -1, -1):
                s = z[k] / d[k]
                for i in range(k + 1, D + 1):
                    s = np.where(i <= deg, s - L[i][k] * a[i], s)
                a[k] = np.where(k <= deg, s, 0.0)
            out.append(a)
    return out[0], out[1], deg, n


def _continuum(a, T, D):
    """acc = a_0; acc = acc + a_k * T_k[c]: -> [R][C]"""
    with np.errstate(all="ignore"):
        acc = np.repeat(a[0][:, None], T.shape[1], axis=1)
        for k in range(1, D + 1):
            acc = acc + a[k][:, None] * T[k][None, :]
    return acc


def _q(w, vre, vim, are, aim, T, D):
    with np.errstate(all="ignore"):
        rre, rim = vre - _continuum(are, T, D), vim - _continuum(aim, T, D)
        return w * (rre * rre + rim * rim)


def contsub(data, x, mask=None, weights=None, degree=1, axis=-1, mode="subtract", nsigma=0.0, niter=0):
    """-> (out, coeffs, info, codes, stats) as Context.contsub returns them, for a two-dimensional `data`: [R][C] for
    axis -1, [C][R] for axis 0; complex128 or float64"""
    data = np.asarray(data)
    assert data.ndim == 2 and data.dtype in (np.complex128, np.float64) and axis in (-1, 0)
    cplx, D = data.dtype == np.complex128, int(degree)
    v = data if axis == -1 else data.T
    R, C = v.shape
    vre = np.ascontiguousarray(v.real, dtype=np.float64)
    vim = np.ascontiguousarray(v.imag, dtype=np.float64) if cplx else np.zeros((R, C))
    x = np.asarray(x, dtype=np.float64)
    T = chebyshev_table(x, D)
    xfin = np.isfinite(x)
    chan = xfin if mask is None else xfin & (np.asarray(mask).astype(np.uint8) != 0)
    codes = np.zeros((R, C), dtype=np.uint8)
    if weights is None:
        w = np.ones((R, C))
    else:
        w = np.ascontiguousarray(weights if axis == -1 else np.asarray(weights).T, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            codes[~(np.isfinite(w) & (w > 0.0))] = FLAGGED
    codes[(codes == 0) & ~(np.isfinite(vre) & np.isfinite(vim))] = NOT_FINITE
    codes[(codes == 0) & ~chan[None, :]] = MASKED
    are, aim, deg, n = _fit(codes == 0, w, vre, vim, T, D)
    clipped = np.zeros(R, dtype=np.int64)
    done = deg < 0
    if nsigma != 0.0:
        lim = np.float64(nsigma) * np.float64(nsigma)
        for i in range(int(niter)):
            if done.all():
                break
            part = (codes == 0) & ~done[:, None]
            q = _q(w, vre, vim, are, aim, T, D)
            Q = np.zeros(R)
            with np.errstate(all="ignore"):
                for c in range(C):
                    Q = np.where(part[:, c], Q + q[:, c], Q)
                limit = lim * (Q / n.astype(np.float64))
                hit = part & (q > limit[:, None])
            codes[hit] = CLIPPED + i
            a2re, a2im, deg2, n2 = _fit(part & ~hit, w, vre, vim, T, D)
            live = ~done
            for k in range(D + 1):
                are[k], aim[k] = np.where(live, a2re[k], are[k]), np.where(live, a2im[k], aim[k])
            deg, n = np.where(live, deg2, deg), np.where(live, n2, n)
            nhit = hit.sum(axis=1)
            clipped = clipped + nhit
            done = done | (nhit == 0) | (deg < 0)
    # the closing pass
    cre, cim = _continuum(are, T, D), _continuum(aim, T, D)
    q = _q(w, vre, vim, are, aim, T, D)
    part = codes == 0
    Q = np.zeros(R)
    with np.errstate(all="ignore"):
        for c in range(C):
            Q = np.where(part[:, c], Q + q[:, c], Q)
        qbar = np.where(n > 0, Q / n.astype(np.float64), np.nan)
        ore, oim = (vre - cre, vim - cim) if mode == "subtract" else (cre, cim)
    ore, oim = np.where(xfin[None, :], ore, np.nan), np.where(xfin[None, :], oim, np.nan)
    if cplx:
        out = np.empty((R, C), dtype=np.complex128)
        out.real, out.imag = ore, oim
        coeffs = np.empty((R, D + 1), dtype=np.complex128)
        coeffs.real, coeffs.imag = np.stack(are, axis=1), np.stack(aim, axis=1)
    else:
        out, coeffs = ore, np.stack(are, axis=1)
    info = np.stack([deg.astype(np.float64), n.astype(np.float64), clipped.astype(np.float64), qbar], axis=1)
    stats = np.array([R, (deg == D).sum(), ((deg >= 0) & (deg < D)).sum(), (deg < 0).sum(), n.sum(), clipped.sum(),
                      (codes == NOT_FINITE).sum(), (codes == FLAGGED).sum()], dtype=np.float64)
    if axis == 0:
        out, coeffs, info, codes = (np.ascontiguousarray(a.T) for a in (out, coeffs, info, codes))
    return np.ascontiguousarray(out), np.ascontiguousarray(coeffs), info, codes, stats


def clip_case(seed, R=200, C=96):
    """Rows of a degree-3 continuum plus noise 0.1 plus a line of height 5 over 8 channels that the mask does not cover.
    -> data [R][C] complex128, x, line (the bool mask [R][C] of the line samples)"""
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.0, 1.0, C)
    a = rng.normal(size=(R, 4)) + 1j * rng.normal(size=(R, 4))
    V = np.stack([np.ones(C), x, 2 * x * x - 1, 4 * x ** 3 - 3 * x])
    data = a @ V + 0.1 * (rng.normal(size=(R, C)) + 1j * rng.normal(size=(R, C)))
    line = np.zeros((R, C), dtype=bool)
    start = rng.integers(4, C - 12, size=R)
    for r in range(R):
        line[r, start[r]:start[r] + 8] = True
    data[line] += 5.0
    return data, x, line
