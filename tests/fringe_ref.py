"""numpy restatement of delay and rate calibration (include/gridhip.h, "delay and rate calibration"): the table, the
fringe search, the antenna-based solve, the driver and the apply step, every rule in the header's order so that - given the
library's table - the search and the solve agree with the device bit for bit.  Moduli are explicit sqrt(re*re + im*im),
never hypot or abs; numpy's element-wise arithmetic does not contract a * b + c."""
import numpy as np

HEAD, ROW = 16, 12
MAX_F, MAX_ND, MAX_TINT, MAX_NR = 1024, 4096, 256, 1024


def table_doubles(F, T, Nd, Nr):
    return HEAD + 2 * F * Nd + 2 * T * Nr + 2 * T + F


def phasor(a, b):
    """exp(2 pi i a b) = (cs, sn), the turns reduced to x - rint(x) first"""
    x = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    r = x - np.rint(x)
    return np.cos(np.pi * (2.0 * r)), np.sin(np.pi * (2.0 * r))


def mulc(x, c):
    """x conj(c) on (re, im) pairs"""
    return x[0] * c[0] + x[1] * c[1], x[1] * c[0] - x[0] * c[1]


def mul(x, c):
    return x[0] * c[0] - x[1] * c[1], x[0] * c[1] + x[1] * c[0]


def mac(acc, e, x):
    """acc + e x as rmsynth adds it"""
    return acc[0] + (e[0] * x[0] - e[1] * x[1]), acc[1] + (e[0] * x[1] + e[1] * x[0])


def intervals(T, tint):
    tint = T if tint == 0 else tint
    return tint, (T + tint - 1) // tint


def tables(freq, time, tint, tau0, dtau, Nd, r0, drate, Nr):
    freq, time = np.asarray(freq, dtype=np.float64), np.asarray(time, dtype=np.float64)
    F, T = len(freq), len(time)
    tint, I = intervals(T, tint)
    out = np.zeros(table_doubles(F, T, Nd, Nr))
    with np.errstate(all="ignore"):
        nu0 = freq[0] + 0.5 * (freq[F - 1] - freq[0])
        valid = bool(np.isfinite(freq).all() and np.isfinite(time).all() and np.isfinite([tau0, dtau, r0, drate, nu0]).all()
                     and dtau > 0.0 and drate > 0.0)
    out[:12] = [float(valid), F, T, tint, I, Nd, Nr, tau0, dtau, r0, drate, nu0 if valid else 0.0]
    if not valid:
        return out
    tref = np.zeros(T)
    for i in range(I):
        ta, tb = i * tint, min(T, (i + 1) * tint)
        tref[i] = time[ta] + 0.5 * (time[tb - 1] - time[ta])
    af = freq - nu0
    dtm = time - tref[np.arange(T) // tint]
    cs, sn = phasor((tau0 + np.arange(Nd) * dtau)[None, :], af[:, None])
    Ef = np.stack([cs, -sn], axis=-1)
    cs, sn = phasor((r0 + np.arange(Nr) * drate)[None, :], dtm[:, None])
    Et = np.stack([cs, -sn], axis=-1)
    out[HEAD:] = np.concatenate([Ef.ravel(), Et.ravel(), tref, af, dtm])
    return out


def split(tb, T, F):
    """the parts of a table, or None when its head does not fit a cube of T time steps and F channels"""
    tb = np.asarray(tb, dtype=np.float64)
    h = tb[:HEAD]
    if not (h[0] == 1.0 and h[1] == F and h[2] == T and 1 <= h[3] <= MAX_TINT and h[3] == int(h[3]) and 1 <= h[5] <= MAX_ND
            and h[5] == int(h[5]) and 1 <= h[6] <= MAX_NR and h[6] == int(h[6])):
        return None
    tint, Nd, Nr = int(h[3]), int(h[5]), int(h[6])
    I = (T + tint - 1) // tint
    if h[4] != I or len(tb) != table_doubles(F, T, Nd, Nr):
        return None
    p = HEAD
    Ef = tb[p:p + 2 * F * Nd].reshape(F, Nd, 2); p += 2 * F * Nd
    Et = tb[p:p + 2 * T * Nr].reshape(T, Nr, 2); p += 2 * T * Nr
    return dict(tint=tint, I=I, Nd=Nd, Nr=Nr, tau0=h[7], dtau=h[8], r0=h[9], drate=h[10], nu0=h[11], Ef=Ef, Et=Et,
                tref=tb[p:p + T], af=tb[p + T:p + T + F], dtm=tb[p + T + F:p + 2 * T + F])


def window(h, wj, wk):
    """the cells within (wj, wk) of the grid's zero"""
    with np.errstate(all="ignore"):
        zj, zk = np.rint(-h["tau0"] / h["dtau"]), np.rint(-h["r0"] / h["drate"])
    zj, zk = (zj if zj > 0.0 else 0.0), (zk if zk > 0.0 else 0.0)
    cj, ck = (int(zj) if zj < h["Nd"] - 1 else h["Nd"] - 1), (int(zk) if zk < h["Nr"] - 1 else h["Nr"] - 1)
    return max(cj - wj, 0), min(cj + wj + 1, h["Nd"]), max(ck - wk, 0), min(ck + wk + 1, h["Nr"])


def derotation(h, sol, i, p, q, t0, nt):
    """d_b, Df[F], Dt[nt] of one (baseline, interval)"""
    sp, sq = sol[i, p], sol[i, q]
    d = mulc((sp[2], sp[3]), (sq[2], sq[3]))
    return d, phasor(sp[0] - sq[0], h["af"]), phasor(sp[1] - sq[1], h["dtm"][t0:t0 + nt])


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
            d, df, dt = derotation(h, sol, i, p, q, t0, nt)
            x = mulc(x, d)
            x = mulc(x, (df[0][None, :], df[1][None, :]))
            x = mulc(x, (dt[0][:, None], dt[1][:, None]))
    return (np.where(flagged, 0.0, x[0]), np.where(flagged, 0.0, x[1])), flagged, t0, nt


def fringe_power(h, x, t0, nt, j0, j1, k0, k1):
    """S[j][k] as (re, im) over the cells by the two ordered sums"""
    F = x[0].shape[1]
    with np.errstate(all="ignore"):
        y = (np.zeros((nt, j1 - j0)), np.zeros((nt, j1 - j0)))
        for f in range(F):
            e = h["Ef"][f, j0:j1]
            y = mac(y, (e[None, :, 0], e[None, :, 1]), (x[0][:, f, None], x[1][:, f, None]))
        s = (np.zeros((j1 - j0, k1 - k0)), np.zeros((j1 - j0, k1 - k0)))
        for t in range(nt):
            e = h["Et"][t0 + t, k0:k1]
            s = mac(s, (e[None, :, 0], e[None, :, 1]), (y[0][t, :, None], y[1][t, :, None]))
    return s


def parabola(pm, ps, pp):
    d = (pm - ps) + (pp - ps)
    return (0.5 * (pm - pp)) / d if d < 0.0 else 0.0


def search(tb, vis, a1, a2, A, model=None, wt=None, sol=None, cells=None):
    """-> (peaks [B][I][12], stats[8]); cells = (j0, j1, k0, k1), None: the whole grid.  A table that does not fit: (None,
    stats with [7] = 1)."""
    B, T, F = vis.shape
    h = split(tb, T, F)
    stats = np.zeros(8)
    if h is not None:
        j0, j1, k0, k1 = (0, h["Nd"], 0, h["Nr"]) if cells is None else cells
        if not (0 <= j0 < j1 <= h["Nd"] and 0 <= k0 < k1 <= h["Nr"]):
            h = None
    if h is None:
        stats[7] = 1.0
        return None, stats
    peaks = np.zeros((B, h["I"], ROW))
    for b in range(B):
        p, q = int(a1[b]), int(a2[b])
        for i in range(h["I"]):
            row = np.array([-1.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
            peaks[b, i] = row
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
                s = fringe_power(h, x, t0, nt, j0, j1, k0, k1)
                with np.errstate(all="ignore"):
                    P = s[0] * s[0] + s[1] * s[1]
                Pm = np.where(np.isnan(P), -1.0, P)
                at = int(np.argmax(Pm))  # (the first of the largest in [j][k] order: lowest j, then lowest k)
                if Pm.ravel()[at] < 0.0:
                    P = None
            if P is None:
                peaks[b, i, 10] = 2.0
                stats[1] += 1
                continue
            jj, kk = divmod(at, k1 - k0)
            ps = P[jj, kk]
            bj, bk = j0 + jj, k0 + kk
            tau, rate = h["tau0"] + float(bj) * h["dtau"], h["r0"] + float(bk) * h["drate"]
            if j0 < bj < j1 - 1:
                tau = tau + parabola(P[jj - 1, kk], ps, P[jj + 1, kk]) * h["dtau"]
            if k0 < bk < k1 - 1:
                rate = rate + parabola(P[jj, kk - 1], ps, P[jj, kk + 1]) * h["drate"]
            N = 0.0
            for t in range(nt):
                e = 0.0
                for f in range(F):
                    e = e + (x[0][t, f] * x[0][t, f] + x[1][t, f] * x[1][t, f])
                N = N + e
            z = (1.0, 0.0)
            if ps > 0.0:
                sq = np.sqrt(ps)
                z = (s[0][jj, kk] / sq, s[1][jj, kk] / sq)
            coh2 = ps / (float(nu) * N) if N > 0.0 else 0.0
            peaks[b, i] = [bj, bk, ps, tau, rate, z[0], z[1], coh2, nu, N, 0.0, 0.0]
            stats[4] += 1
    return peaks, stats


def weights(peaks, a1, a2, A, i, min_count, min_coh2):
    B = peaks.shape[0]
    w = np.zeros(B)
    for b in range(B):
        row, p, q = peaks[b, i], int(a1[b]), int(a2[b])
        use = (row[10] == 0.0 and row[8] >= min_count and row[7] >= min_coh2 and row[7] > 0.0
               and np.isfinite(row[[3, 4, 5, 6, 7]]).all() and 0 <= p < A and 0 <= q < A and p != q)
        w[b] = row[7] if use else 0.0
    return w


def solve(peaks, a1, a2, A, sol, min_count=0.0, min_coh2=0.0, refant=0, niter=50, tol=0.0):
    """-> (sol accumulated into a copy, info [I][A], stats[8])"""
    B, I = peaks.shape[:2]
    sol = np.array(sol, dtype=np.float64)
    info = np.zeros((I, A))
    part = np.zeros((I, 8))
    refant = -1 if refant is None or refant < 0 else int(refant)
    for i in range(I):
        w = weights(peaks, a1, a2, A, i, min_count, min_coh2)
        used = [b for b in range(B) if w[b] > 0.0]
        cnt = np.zeros(A, dtype=int)
        for b in used:
            cnt[int(a1[b])] += 1
            cnt[int(a2[b])] += 1
        xt, xr = np.zeros(A), np.zeros(A)
        hr, hi = np.ones(A), np.zeros(A)
        iters = 0
        for it in range(niter):
            nxt, nxr, nhr, nhi = xt.copy(), xr.copy(), hr.copy(), hi.copy()
            ct = st = cr = sr = ch = 0.0
            for s in range(A):
                if cnt[s] == 0:
                    continue
                den = nt = nr = 0.0
                num = (0.0, 0.0)
                for b in used:
                    p, q = int(a1[b]), int(a2[b])
                    if p != s and q != s:
                        continue
                    row, wb = peaks[b, i], w[b]
                    wz = (wb * row[5], wb * row[6])
                    den = den + wb
                    if p == s:
                        nt = nt + wb * (row[3] + xt[q])
                        nr = nr + wb * (row[4] + xr[q])
                        num = (num[0] + (wz[0] * hr[q] - wz[1] * hi[q]), num[1] + (wz[0] * hi[q] + wz[1] * hr[q]))
                    else:
                        nt = nt + wb * (xt[p] - row[3])
                        nr = nr + wb * (xr[p] - row[4])
                        num = (num[0] + (wz[0] * hr[p] + wz[1] * hi[p]), num[1] + (wz[0] * hi[p] - wz[1] * hr[p]))
                t1, r1 = nt / den, nr / den
                g = (hr[s], hi[s])
                m2 = num[0] * num[0] + num[1] * num[1]
                if m2 > 0.0 and np.isfinite(m2):
                    sq = np.sqrt(m2)
                    g = (num[0] / sq, num[1] / sq)
                if it & 1:
                    t1, r1 = 0.5 * (t1 + xt[s]), 0.5 * (r1 + xr[s])
                    av = (0.5 * (g[0] + hr[s]), 0.5 * (g[1] + hi[s]))
                    n2 = av[0] * av[0] + av[1] * av[1]
                    if n2 > 0.0 and np.isfinite(n2):
                        sq = np.sqrt(n2)
                        g = (av[0] / sq, av[1] / sq)
                    else:
                        g = (hr[s], hi[s])
                nxt[s], nxr[s], nhr[s], nhi[s] = t1, r1, g[0], g[1]
                dx, dy = g[0] - hr[s], g[1] - hi[s]
                ct, st = max(ct, abs(t1 - xt[s])), max(st, abs(t1))
                cr, sr = max(cr, abs(r1 - xr[s])), max(sr, abs(r1))
                ch = max(ch, np.sqrt(dx * dx + dy * dy))
            xt, xr, hr, hi = nxt, nxr, nhr, nhi
            iters += 1
            if ct <= tol * st and cr <= tol * sr and ch <= tol:
                break
        ref_ok = refant >= 0 and cnt[refant] > 0
        reft, refr, refh = (xt[refant], xr[refant], (hr[refant], hi[refant])) if refant >= 0 else (0.0, 0.0, (1.0, 0.0))
        for s in range(A):
            info[i, s] = cnt[s]
            if cnt[s] == 0:
                continue
            t1, r1, g1 = xt[s], xr[s], (hr[s], hi[s])
            if ref_ok:
                t1, r1 = t1 - reft, r1 - refr
                g1 = (1.0, 0.0) if s == refant else mulc(g1, refh)
            sol[i, s, 0] = sol[i, s, 0] + t1
            sol[i, s, 1] = sol[i, s, 1] + r1
            g = mul((sol[i, s, 2], sol[i, s, 3]), g1)
            m2 = g[0] * g[0] + g[1] * g[1]
            if m2 > 0.0 and np.isfinite(m2):
                sq = np.sqrt(m2)
                g = (g[0] / sq, g[1] / sq)
            sol[i, s, 2], sol[i, s, 3] = g
        run = (B + 255) // 256
        runs = np.zeros((3, 256))
        for c in range(256):
            sw = swt = swr = 0.0
            for b in range(c * run, min(B, (c + 1) * run)):
                if w[b] > 0.0:
                    row = peaks[b, i]
                    sw, swt, swr = sw + w[b], swt + w[b] * (row[3] * row[3]), swr + w[b] * (row[4] * row[4])
            runs[:, c] = sw, swt, swr
        tot = [0.0, 0.0, 0.0]
        for c in range(256):
            tot = [tot[0] + runs[0, c], tot[1] + runs[1, c], tot[2] + runs[2, c]]
        part[i] = [iters, len(used), int((cnt == 0).sum()), float(refant >= 0 and not ref_ok), tot[0], tot[1], tot[2], 0.0]
    stats = np.zeros(8)
    sw = swt = swr = 0.0
    for i in range(I):
        stats[0] = max(stats[0], part[i, 0])
        stats[1], stats[2], stats[3] = stats[1] + part[i, 1], stats[2] + part[i, 2], stats[3] + part[i, 3]
        sw, swt, swr = sw + part[i, 4], swt + part[i, 5], swr + part[i, 6]
    if sw > 0.0:
        stats[4], stats[5] = np.sqrt(swt / sw), np.sqrt(swr / sw)
    return sol, info, stats


def fringefit(tb, vis, a1, a2, A, model=None, wt=None, sol=None, rounds=3, window_cells=(2, 2), min_count=0.0, min_coh2=0.0,
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
    stats[:7] = [vs[0], ss[0], ss[1], ss[2], vs[2], vs[4] / h["dtau"], vs[5] / h["drate"]]
    return cur, peaks, info, stats


def apply(tb, sol, a1, a2, vis, wt=None, inverse=True):
    """-> (vis_out, wt_out)"""
    B, T, F = vis.shape
    h = split_head(tb, T, F)
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
            d, df, dt = derotation(h, sol, i, p, q, t0, nt)
            df, dt = (df[0][None, :], df[1][None, :]), (dt[0][:, None], dt[1][:, None])
            v = vis[b, t0:t0 + nt]
            x = (v.real, v.imag)
            x = mulc(mulc(mulc(x, d), df), dt) if inverse else mul(mul(mul(x, d), df), dt)
            out[b, t0:t0 + nt] = x[0] + 1j * x[1]
    return out, wout


def split_head(tb, T, F):
    """what apply reads of a table: the head, a[F] and dt[T] (any Nd, Nr)"""
    tb = np.asarray(tb, dtype=np.float64)
    tint, Nd, Nr = int(tb[3]), int(tb[5]), int(tb[6])
    p = HEAD + 2 * F * Nd + 2 * T * Nr
    return dict(tint=tint, I=(T + tint - 1) // tint, af=tb[p + T:p + T + F], dtm=tb[p + T + F:p + 2 * T + F])


def fringe_grid(freq, time, tint, pad=4):
    """the grid gridhip.fringe_grid proposes, restated"""
    freq, time = np.asarray(freq, dtype=np.float64), np.asarray(time, dtype=np.float64)
    F, T = len(freq), len(time)
    tint, _ = intervals(T, tint)
    df = float(np.median(np.abs(np.diff(freq)))) if F > 1 else 1.0
    dt = float(np.median(np.abs(np.diff(time)))) if T > 1 else 1.0
    Nd, Nr = pad * F, pad * tint
    dtau, drate = 1.0 / (pad * F * df), 1.0 / (pad * tint * dt)
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nr // 2) * drate, drate, Nr)
