"""Rotation-measure synthesis and RM-CLEAN in numpy, statement by statement as include/gridhip.h ("rotation-measure
synthesis") defines them.  numpy never fuses a multiply with an add, so every "rounded" product and bracket of the header
is one numpy operation here, and from a given table on the bits are the library's: synth and rmclean take the table the
library made.  The table itself is the one place where bits cannot match - the device's sincospi and exp are not numpy's -
so `tables` is the header's recipe with numpy's functions (for tests without a device) and `check_tables` compares a table
with long-double values inside the bounds written at each assertion."""
import math

import numpy as np

HEAD, MAPS, STATS = 16, 7, 8
MAX_C, MAX_J = 1024, 512
INV_PI = 0.3183098861837907
FOUR_LN2 = 2.772588722239781
U = 2.0 ** -53
f64, c128 = np.float64, np.complex128


def table_doubles(C, J):
    return HEAD + 2 * C * J + 3 * (2 * J - 1)


def parts(tab, C, J):
    """head, E[C][J], R[2J - 1], G[2J - 1] of a table (copies)"""
    tab = np.asarray(tab, dtype=f64)
    assert tab.shape == (table_doubles(C, J),)
    nE, nL = C * J, 2 * J - 1
    E = tab[HEAD:HEAD + 2 * nE].reshape(C, J, 2)
    R = tab[HEAD + 2 * nE:HEAD + 2 * nE + 2 * nL].reshape(nL, 2)
    return tab[:HEAD].copy(), E[..., 0] + 1j * E[..., 1], R[:, 0] + 1j * R[:, 1], tab[HEAD + 2 * nE + 2 * nL:].copy()


def head_of(lam2, weights, phi0, dphi, J, fwhm):
    """the 16 values of the head: plain ascending sums in Python floats, every product rounded"""
    C = len(lam2)
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=f64)
    sw = swl = 0.0
    ok = True
    for c in range(C):
        wc, l = float(w[c]), float(lam2[c])
        ok = ok and math.isfinite(l) and math.isfinite(wc) and wc >= 0.0
        sw = sw + wc
        swl = swl + wc * l
    ok = ok and math.isfinite(sw) and sw > 0.0 and math.isfinite(swl)
    head = np.zeros(HEAD)
    head[:5] = [1.0 if ok else 0.0, C, J, phi0, dphi]
    head[8] = fwhm
    if ok:
        head[5], head[6], head[7] = swl / sw, 1.0 / sw, sw
    return head


def _phasor(x, a, kw):
    t = (x * a) * INV_PI
    r = t - np.rint(t)
    ang = np.pi * (2.0 * r)
    return kw * np.cos(ang), -(kw * np.sin(ang))


def tables(lam2, weights, phi0, dphi, J, fwhm):
    """the header's recipe with numpy's sin, cos and exp in place of sincospi and exp of the device"""
    lam2 = np.asarray(lam2, dtype=f64)
    C = len(lam2)
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=f64)
    head = head_of(lam2, weights, phi0, dphi, J, fwhm)
    tab = np.zeros(table_doubles(C, J))
    tab[:HEAD] = head
    if head[0] != 1.0:
        return tab
    lam0, K = head[5], head[6]
    a, kw = lam2 - lam0, K * w
    phi = phi0 + np.arange(J, dtype=f64) * dphi
    ere, eim = _phasor(phi[None, :], a[:, None], kw[:, None])
    lag = np.arange(-(J - 1), J, dtype=f64) * dphi
    sre, sim = np.zeros(2 * J - 1), np.zeros(2 * J - 1)
    for c in range(C):
        tre, tim = _phasor(lag, a[c], kw[c])
        sre, sim = sre + tre, sim + tim
    x = lag / fwhm
    G = np.exp(-(FOUR_LN2 * (x * x)))
    nE, nL = C * J, 2 * J - 1
    tab[HEAD:HEAD + 2 * nE] = np.stack([ere, eim], axis=-1).reshape(-1)
    tab[HEAD + 2 * nE:HEAD + 2 * nE + 2 * nL] = np.stack([sre, sim], axis=-1).reshape(-1)
    tab[HEAD + 2 * nE + 2 * nL:] = G
    return tab


def check_tables(tab, lam2, weights, phi0, dphi, J, fwhm):
    """A table of the library against long-double values.  Exact: the head (Python's ascending sums), Im R[J - 1] == 0,
    G[J - 1] == 1, and all zeros behind the head when valid = 0.  Within bounds, u = 2^-53:
      E   16 u (max |phi a| + 1) kw_c: four roundings of a phase (phi_j, a_c, the product, the division by pi) are
          8 u |phi a| radians, sincospi a few ulp on top, and a margin of 2 over both;
      R   16 u (max |lag a| + 1) + 2 C u: the same per term (the kw_c sum to 1) and the C additions;
      G   8 u (1 + |x|) relative, x its exponent: the roundings of x scale with |x|, exp adds an ulp or two."""
    ld = np.longdouble
    lam2 = np.asarray(lam2, dtype=f64)
    C = len(lam2)
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=f64)
    head, E, R, G = parts(tab, C, J)
    want = head_of(lam2, weights, phi0, dphi, J, fwhm)
    assert np.array_equal(head, want), (head, want)
    if head[0] != 1.0:
        assert not np.any(np.asarray(tab)[HEAD:] != 0.0)
        return
    lam0, K = head[5], head[6]
    a = lam2.astype(ld) - ld(lam0)
    kw = K * w  # (as the device forms it; its own rounding is inside the "+ 1")
    phi = ld(phi0) + np.arange(J).astype(ld) * ld(dphi)
    ang = -2 * phi[None, :] * a[:, None]
    ref = kw[:, None].astype(ld) * (np.cos(ang) + 1j * np.sin(ang))
    bound = 16 * U * (float(np.abs(phi[None, :] * a[:, None]).max()) + 1.0) * kw[:, None]
    err = np.abs((E.real.astype(ld) - ref.real) + 1j * (E.imag.astype(ld) - ref.imag)).astype(f64)
    assert np.all(err <= bound), f"E: {float((err / np.maximum(bound, 1e-300)).max())} of the bound"
    lag = np.arange(-(J - 1), J).astype(ld) * ld(dphi)
    ang = -2 * lag[None, :] * a[:, None]
    ref = (kw[:, None].astype(ld) * (np.cos(ang) + 1j * np.sin(ang))).sum(axis=0)
    bound = 16 * U * (float(np.abs(lag[None, :] * a[:, None]).max()) + 1.0) + 2 * C * U
    err = np.abs((R.real.astype(ld) - ref.real) + 1j * (R.imag.astype(ld) - ref.imag)).astype(f64)
    assert np.all(err <= bound), f"R: {float(err.max() / bound)} of the bound"
    assert R[J - 1].imag == 0.0 and G[J - 1] == 1.0
    x = -ld(4) * np.log(ld(2)) * (lag / ld(fwhm)) ** 2
    ref = np.exp(x)
    rel = np.abs(G.astype(ld) - ref).astype(f64)
    assert np.all(rel <= 8 * U * (1.0 + np.abs(x).astype(f64)) * ref.astype(f64) + 5e-324), "G"


def table_fits(tab, C, J):
    """rm_head_ok of csrc/rm.hip: C None - any C in range"""
    hc = tab[1]
    return bool(tab[0] == 1.0 and 1.0 <= hc <= MAX_C and hc == int(hc) and tab[2] == J and (C is None or hc == C))


def synth(tab, Q, U_):
    """Q, U [C][M] -> (cube [J][M], stats) as gridhip_rmsynth leaves them; None for the cube when the table does not fit"""
    Q, U_ = np.asarray(Q, dtype=f64), np.asarray(U_, dtype=f64)
    C, M = Q.shape
    J = int(tab[2])
    stats = np.zeros(STATS)
    if not table_fits(tab, C, J):
        stats[7] = 1.0
        return None, stats
    _, E, _, _ = parts(tab, C, J)
    re, im = np.zeros((J, M)), np.zeros((J, M))
    with np.errstate(all="ignore"):
        for c in range(C):
            er, ei, q, u = E[c].real[:, None], E[c].imag[:, None], Q[c][None, :], U_[c][None, :]
            re = re + (er * q - ei * u)
            im = im + (er * u + ei * q)
    bad = ~(np.isfinite(Q).all(axis=0) & np.isfinite(U_).all(axis=0))
    re[:, bad], im[:, bad] = np.nan, np.nan
    stats[0] = bad.sum()
    return re + 1j * im, stats


def _argmax(re, im):
    """(p_k, k): the largest p, ties to the lowest depth, a NaN never; (-1, -1) when every p is NaN"""
    with np.errstate(all="ignore"):
        p = re * re + im * im
    p = np.where(np.isnan(p), -1.0, p)
    k = int(np.argmax(p))
    return (float(p[k]), k, p) if p[k] >= 0.0 else (-1.0, -1, p)


def rmclean(tab, cube, model=None, gain=0.1, threshold=0.0, niter=100, nsigma=0.0, noise=None, restore=False):
    """-> (model, cube, maps, stats, gap): copies as gridhip_rmclean leaves the arrays ([J][M]), and the smallest relative
    gap between the two largest p that any component was chosen at (inf when none was, or J == 1)."""
    cube = np.array(cube, dtype=c128)
    J, M = cube.shape
    model = np.zeros((J, M), dtype=c128) if model is None else np.array(model, dtype=c128)
    maps, stats, gap = np.full((MAPS, M), np.nan), np.zeros(STATS), np.inf
    L = float(threshold)
    if nsigma > 0.0:
        sigma = float(np.asarray(noise).reshape(-1)[0])
        if sigma != sigma:
            stats[6] = 1.0
            return model, cube, None, stats, gap
        a = nsigma * sigma
        L = a if a > L else L
    if not table_fits(tab, None, J):
        stats[7] = 1.0
        return model, cube, None, stats, gap
    C = int(tab[1])
    head, _, R, G = parts(tab, C, J)
    phi0, dphi = head[3], head[4]
    L2 = L * L
    jj = np.arange(J)
    for m in range(M):
        re, im = cube[:, m].real.copy(), cube[:, m].imag.copy()
        if not (np.isfinite(re).all() and np.isfinite(im).all()):
            maps[:, m] = [0.0, 3.0, -1.0, np.nan, np.nan, np.nan, np.nan]
            stats[0] += 1
            continue
        mre, mim = model[:, m].real.copy(), model[:, m].imag.copy()
        it = 0
        with np.errstate(all="ignore"):
            while True:
                pk, k, p = _argmax(re, im)
                if pk <= L2:
                    reason = 1
                    break
                if it >= niter:
                    reason = 0
                    break
                if J > 1:
                    top = np.sort(p)[-2:]
                    gap = min(gap, float((top[1] - top[0]) / top[1]))
                fr, fi = gain * re[k], gain * im[k]
                mre[k], mim[k] = mre[k] + fr, mim[k] + fi
                r = R[jj - k + J - 1]
                re = re - (fr * r.real - fi * r.imag)
                im = im - (fr * r.imag + fi * r.real)
                it += 1
            if restore:
                for k in range(J):
                    if mre[k] != 0.0 or mim[k] != 0.0:
                        g = G[jj - k + J - 1]
                        re = re + mre[k] * g
                        im = im + mim[k] * g
            ps, js, p = _argmax(re, im)
            if js >= 0:
                phi = phi0 + float(js) * dphi
                fit = phi
                if 0 < js < J - 1:
                    pm, pp = re[js - 1] * re[js - 1] + im[js - 1] * im[js - 1], re[js + 1] * re[js + 1] + im[js + 1] * im[js + 1]
                    d = (pm - ps) + (pp - ps)
                    if d < 0.0:
                        off = (0.5 * (pm - pp)) / d
                        fit = phi + off * dphi
                maps[:, m] = [it, reason, js, ps, fit, re[js], im[js]]
            else:
                maps[:, m] = [it, reason, -1.0, np.nan, np.nan, np.nan, np.nan]
        stats[1] += it
        stats[2] += reason == 0
        stats[3] += reason == 1
        cube[:, m], model[:, m] = re + 1j * im, mre + 1j * mim
    stats[5] = L
    return model, cube, maps, stats, gap


def sky(rng, lam2, phi0, dphi, J, M, ncomp=(1, 3), noise=0.02, edge=False):
    """Q, U [C][M] of M lines of sight with 1 to 3 Faraday-thin components on grid depths (edge: the first line of sight
    has them at depth 0 and J - 1) plus Gaussian noise; -> Q, U, the list of (depths, amplitudes) per line of sight"""
    lam2 = np.asarray(lam2, dtype=f64)
    C = len(lam2)
    P = np.zeros((C, M), dtype=c128)
    truth = []
    for m in range(M):
        n = int(rng.integers(ncomp[0], ncomp[1] + 1))
        js = rng.choice(J, size=min(n, J), replace=False)
        if edge and m == 0:
            js = np.array([0, J - 1][:max(1, min(2, J))])
        amp = rng.uniform(0.5, 1.5, len(js)) * np.exp(2j * rng.uniform(0, np.pi, len(js)))
        for j, a in zip(js, amp):
            P[:, m] += a * np.exp(2j * (phi0 + j * dphi) * lam2)
        truth.append((js, amp))
    P += noise * (rng.normal(size=(C, M)) + 1j * rng.normal(size=(C, M)))
    return np.ascontiguousarray(P.real), np.ascontiguousarray(P.imag), truth
