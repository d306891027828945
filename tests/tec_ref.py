"""numpy restatement of dispersive delay (TEC) calibration (include/gridhip.h, "dispersive delay (TEC) calibration"): the
table, the delay-TEC search, the driver and the apply step, one rounded operation at a time in the header's order, so that
- given the library's table - the search agrees with the device bit for bit.  The antenna fit is fringe_ref.solve,
unchanged.  numpy's element-wise arithmetic does not contract a * b + c."""
import numpy as np

from fringe_ref import intervals, mac, mul, mulc, parabola, phasor, solve

KAPPA = 1.3445365934456e9
HEAD, ROW = 16, 12
MAX_F, MAX_ND, MAX_NM = 1024, 4096, 1024


def table_doubles(F, Nd, Nm):
    return HEAD + 2 * F * Nd + 2 * F * Nm + 2 * F


def coordinates(freq, orthogonal=True):
    """nu0, a[F], c[F], s by the header's rounded rules; orthogonal=False forces s = 0 (the raw dispersive axis)"""
    freq = np.asarray(freq, dtype=np.float64)
    F = len(freq)
    with np.errstate(all="ignore"):
        nu0 = freq[0] + 0.5 * (freq[F - 1] - freq[0])
        a = freq - nu0
        z = -(KAPPA * (1.0 / freq - 1.0 / nu0))
        num = den = 0.0
        for f in range(F):
            num, den = num + a[f] * z[f], den + a[f] * a[f]
        s = num / den if den > 0.0 else 0.0
        if not orthogonal:
            s = 0.0
        c = z - s * a
    return nu0, a, c, s


def tables(freq, T, tint, tau0, dtau, Nd, tec0, dtec, Nm, orthogonal=True):
    freq = np.asarray(freq, dtype=np.float64)
    F = len(freq)
    tint, I = intervals(T, tint)
    out = np.zeros(table_doubles(F, Nd, Nm))
    with np.errstate(all="ignore"):
        good = bool(np.isfinite(freq).all() and (freq > 0.0).all())
        nu0, a, c, s = coordinates(freq, orthogonal) if good else (0.0, None, None, 0.0)
        valid = bool(good and np.isfinite([tau0, dtau, tec0, dtec, nu0, s]).all() and dtau > 0.0 and dtec > 0.0)
    out[:14] = [float(valid), F, T, tint, I, Nd, Nm, tau0, dtau, tec0, dtec, nu0 if valid else 0.0, s if valid else 0.0, KAPPA]
    if not valid:
        return out
    cs, sn = phasor((tau0 + np.arange(Nd) * dtau)[None, :], a[:, None])
    Ef = np.stack([cs, -sn], axis=-1)
    cs, sn = phasor((tec0 + np.arange(Nm) * dtec)[None, :], c[:, None])
    Em = np.stack([cs, -sn], axis=-1)
    out[HEAD:] = np.concatenate([Ef.ravel(), Em.ravel(), a, c])
    return out


def split(tb, T, F, whole=True):
    """the parts of a table, or None when its head does not fit a cube of T time steps and F channels"""
    tb = np.asarray(tb, dtype=np.float64)
    h = tb[:HEAD]
    if not (h[0] == 1.0 and h[1] == F and h[2] == T and T >= 1 and 1 <= h[3] <= T and h[3] == int(h[3]) and 1 <= h[5] <= MAX_ND
            and h[5] == int(h[5]) and 1 <= h[6] <= MAX_NM and h[6] == int(h[6]) and 1 <= F <= MAX_F):
        return None
    tint, Nd, Nm = int(h[3]), int(h[5]), int(h[6])
    I = (T + tint - 1) // tint
    if h[4] != I or (whole and len(tb) != table_doubles(F, Nd, Nm)):
        return None
    p = HEAD
    Ef = tb[p:p + 2 * F * Nd].reshape(F, Nd, 2); p += 2 * F * Nd
    Em = tb[p:p + 2 * F * Nm].reshape(F, Nm, 2); p += 2 * F * Nm
    return dict(tint=tint, I=I, Nd=Nd, Nm=Nm, tau0=h[7], dtau=h[8], tec0=h[9], dtec=h[10], nu0=h[11], s=h[12], Ef=Ef, Em=Em,
                af=tb[p:p + F], cf=tb[p + F:p + 2 * F])


def window(h, wj, wm):
    """the cells within (wj, wm) of the grid's zero"""
    with np.errstate(all="ignore"):
        zj, zm = np.rint(-h["tau0"] / h["dtau"]), np.rint(-h["tec0"] / h["dtec"])
    zj, zm = (zj if zj > 0.0 else 0.0), (zm if zm > 0.0 else 0.0)
    cj, cm = (int(zj) if zj < h["Nd"] - 1 else h["Nd"] - 1), (int(zm) if zm < h["Nm"] - 1 else h["Nm"] - 1)
    return max(cj - wj, 0), min(cj + wj + 1, h["Nd"]), max(cm - wm, 0), min(cm + wm + 1, h["Nm"])


def derotation(h, sol, i, p, q):
    """d_b and Dfm[F] of one (baseline, interval)"""
    sp, sq = sol[i, p], sol[i, q]
    d = mulc((sp[2], sp[3]), (sq[2], sq[3]))
    return d, mul(phasor(sp[0] - sq[0], h["af"]), phasor(sp[1] - sq[1], h["cf"]))


def samples(h, vis, model, wt, sol, b, i, p, q):
    """X' [nt, F] as (re, im), and the mask of the flagged samples"""
    t0 = i * h["tint"]
    nt = min(h["tint"], vis.shape[1] - t0)
    v = vis[b, t0:t0 + nt]
    s = np.ones(v.shape) if wt is None else wt[b, t0:t0 + nt]
    with np.errstate(all="ignore"):
        flagged = ~(s > 0.0)
        x = (s * v.real, s * v.imag)
        if model is not None:
            m = model[b, t0:t0 + nt]
            x = mulc(x, (m.real, m.imag))
        if sol is not None:
            d, dfm = derotation(h, sol, i, p, q)
            x = mulc(mulc(x, d), (dfm[0][None, :], dfm[1][None, :]))
    return (np.where(flagged, 0.0, x[0]), np.where(flagged, 0.0, x[1])), flagged, t0, nt


def xbar(x):
    """sum_t X'[t][f], t ascending from (0, 0)"""
    re, im = np.zeros(x[0].shape[1]), np.zeros(x[0].shape[1])
    with np.errstate(all="ignore"):
        for t in range(x[0].shape[0]):
            re, im = re + x[0][t], im + x[1][t]
    return re, im


def power_sums(h, xb, j0, j1, m0, m1):
    """S[j][m] as (re, im) over the cells by the ordered sum"""
    F = len(xb[0])
    s = (np.zeros((j1 - j0, m1 - m0)), np.zeros((j1 - j0, m1 - m0)))
    with np.errstate(all="ignore"):
        for f in range(F):
            em = h["Em"][f, m0:m1]
            pr = mul((em[:, 0], em[:, 1]), (xb[0][f], xb[1][f]))
            e = h["Ef"][f, j0:j1]
            s = mac(s, (e[:, None, 0], e[:, None, 1]), (pr[0][None, :], pr[1][None, :]))
    return s


def search(tb, vis, a1, a2, A, model=None, wt=None, sol=None, cells=None):
    """-> (peaks [B][I][12], stats[8]); cells = (j0, j1, m0, m1), None: the whole grid.  A table that does not fit: (None,
    stats with [7] = 1)."""
    B, T, F = vis.shape
    h = split(tb, T, F)
    stats = np.zeros(8)
    if h is not None:
        j0, j1, m0, m1 = (0, h["Nd"], 0, h["Nm"]) if cells is None else cells
        if not (0 <= j0 < j1 <= h["Nd"] and 0 <= m0 < m1 <= h["Nm"]):
            h = None
    if h is None:
        stats[7] = 1.0
        return None, stats
    peaks = np.zeros((B, h["I"], ROW))
    for b in range(B):
        p, q = int(a1[b]), int(a2[b])
        for i in range(h["I"]):
            peaks[b, i] = [-1.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
            if not (0 <= p < A and 0 <= q < A and p != q):
                peaks[b, i, 10] = 3.0
                stats[3] += 1
                continue
            x, flagged, t0, nt = samples(h, vis, model, wt, sol, b, i, p, q)
            nu = int((~flagged).sum())
            stats[0] += int(flagged.sum())
            peaks[b, i, 8] = nu
            if nu == 0:
                peaks[b, i, 10] = 1.0
                stats[2] += 1
                continue
            P = None
            if np.isfinite(x[0]).all() and np.isfinite(x[1]).all():
                s = power_sums(h, xbar(x), j0, j1, m0, m1)
                with np.errstate(all="ignore"):
                    P = s[0] * s[0] + s[1] * s[1]
                Pm = np.where(np.isnan(P), -1.0, P)
                at = int(np.argmax(Pm))  # (the first of the largest in [j][m] order: lowest j, then lowest m)
                if Pm.ravel()[at] < 0.0:
                    P = None
            if P is None:
                peaks[b, i, 10] = 2.0
                stats[1] += 1
                continue
            jj, mm = divmod(at, m1 - m0)
            ps = P[jj, mm]
            bj, bm = j0 + jj, m0 + mm
            tau, tec = h["tau0"] + float(bj) * h["dtau"], h["tec0"] + float(bm) * h["dtec"]
            if j0 < bj < j1 - 1:
                tau = tau + parabola(P[jj - 1, mm], ps, P[jj + 1, mm]) * h["dtau"]
            if m0 < bm < m1 - 1:
                tec = tec + parabola(P[jj, mm - 1], ps, P[jj, mm + 1]) * h["dtec"]
            N = 0.0
            for t in range(nt):
                e = 0.0
                for f in range(F):
                    e = e + (x[0][t, f] * x[0][t, f] + x[1][t, f] * x[1][t, f])
                N = N + e
            z = (1.0, 0.0)
            if ps > 0.0:
                sq = np.sqrt(ps)
                z = (s[0][jj, mm] / sq, s[1][jj, mm] / sq)
            coh2 = ps / (float(nu) * N) if N > 0.0 else 0.0
            peaks[b, i] = [bj, bm, ps, tau, tec, z[0], z[1], coh2, nu, N, 0.0, 0.0]
            stats[4] += 1
    return peaks, stats


def tecfit(tb, vis, a1, a2, A, model=None, wt=None, sol=None, rounds=3, window_cells=(2, 2), min_count=0.0, min_coh2=0.0,
           refant=0, niter=50, tol=0.0, history=None):
    """-> (sol, peaks, info, stats); history: a list that gets (peaks, sol) of every round"""
    B, T, F = vis.shape
    h = split(tb, T, F)
    stats = np.zeros(8)
    if h is None:
        stats[7] = 1.0
        return None, None, None, stats
    warm = sol is not None
    cur = np.array(sol, dtype=np.float64) if warm else np.tile([0.0, 0.0, 1.0, 0.0], (h["I"], A, 1))
    for r in range(rounds):
        cells = None if r == 0 else window(h, *window_cells)
        peaks, ss = search(tb, vis, a1, a2, A, model, wt, cur if (warm or r > 0) else None, cells)
        cur, info, vs = solve(peaks, a1, a2, A, cur, min_count, min_coh2, refant, niter, tol)
        if history is not None:
            history.append((peaks, cur.copy()))
    stats[:7] = [vs[0], ss[0], ss[1], ss[2], vs[2], vs[4] / h["dtau"], vs[5] / h["dtec"]]
    return cur, peaks, info, stats


def apply(tb, sol, a1, a2, vis, wt=None, inverse=True):
    """-> (vis_out, wt_out)"""
    B, T, F = vis.shape
    h = split(tb, T, F, whole=False)
    A = sol.shape[1]
    out = np.array(vis, dtype=np.complex128)
    wout = np.ones(vis.shape) if wt is None else np.array(wt, dtype=np.float64)
    for b in range(B):
        p, q = int(a1[b]), int(a2[b])
        for i in range(h["I"]):
            t0 = i * h["tint"]
            nt = min(h["tint"], T - t0)
            if not (0 <= p < A and 0 <= q < A and np.isfinite(sol[i, p]).all() and np.isfinite(sol[i, q]).all()):
                wout[b, t0:t0 + nt] = 0.0
                continue
            d, dfm = derotation(h, sol, i, p, q)
            dfm = (dfm[0][None, :], dfm[1][None, :])
            v = vis[b, t0:t0 + nt]
            x = (v.real, v.imag)
            x = mulc(mulc(x, d), dfm) if inverse else mul(mul(x, d), dfm)
            out[b, t0:t0 + nt] = x[0] + 1j * x[1]
    return out, wout


def tec_grid(freq, tec_max, pad=4):
    """the grid gridhip.tec_grid proposes, restated"""
    freq = np.asarray(freq, dtype=np.float64)
    F = len(freq)
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    a, z = freq - nu0, -(KAPPA * (1.0 / freq - 1.0 / nu0))
    c = z - (float((a * z).sum()) / float((a * a).sum())) * a
    df = float(np.median(np.abs(np.diff(freq))))
    Nd, dtau, dtec = pad * F, 1.0 / (pad * F * df), 1.0 / (pad * float(c.max() - c.min()))
    Nm = 2 * int(np.ceil(tec_max / dtec)) + 1
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nm // 2) * dtec, dtec, Nm)
