"""Source finding restated in numpy, step by step as include/gridhip.h ("source finding") defines it: the islands by
automask_ref's flood fill and the hysteresis rule, the sums in plain row-major order, the derived fields in the header's
order.  The reference the find_sources tests compare the library with."""
import math

import numpy as np

import automask_ref
import noise_ref

COMP, INFO = 10, 16
LN2 = 0.693147180559945309417


def beam_usable(beam):
    A, B, C, ok = (float(beam[i]) for i in (0, 1, 2, 7))
    return (ok != 0.0 and ok == ok and 0.0 < A < math.inf and 0.0 < C < math.inf and -math.inf < B < math.inf
            and A * C - B * B > 0.0)


def beam_covariance(beam):
    """(bxx, bxy, byy) of exp(-(A dx^2 + 2 B dx dy + C dy^2))"""
    A, B, C = (float(beam[i]) for i in (0, 1, 2))
    two = 2.0 * (A * C - B * B)
    return C / two, -B / two, A / two


def islands(image, sigma=None, border=0, thr=(0.0, 0.0), nsigma=(5.0, 2.5), peak_frac=0.0, min_cells=1):
    """auto-masking's levels and steps 1-3 without `absolute` -> (T_hi, T_lo, P, reason, labels of L, K)"""
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    region = np.zeros((N, N), dtype=bool)
    region[border:N - border, border:N - border] = True
    part = region & np.isfinite(image)
    T_hi, T_lo = float(thr[0]), float(thr[1])
    P = np.nan
    if part.any():
        P = float(noise_ref.values(noise_ref.keys(image[part]).max(keepdims=True))[0])
    if nsigma[0] > 0.0:
        sigma = float(sigma)
        if sigma != sigma:
            return np.nan, np.nan, P, 3, None, None
        T_hi = max(T_hi, float(np.float64(nsigma[0]) * np.float64(sigma)))
        if nsigma[1] > 0.0:
            T_lo = max(T_lo, float(np.float64(nsigma[1]) * np.float64(sigma)))
    if not part.any():
        return T_hi, T_lo, P, 2, None, None
    if peak_frac > 0.0:
        c = float(np.float64(peak_frac) * np.float64(P))
        T_hi, T_lo = max(T_hi, c), max(T_lo, c)
    with np.errstate(invalid="ignore"):
        Hs, Ls = part & (image > T_hi), part & (image > T_lo)
    lh = automask_ref.label(Hs)
    roots, sizes = np.unique(lh[lh >= 0], return_counts=True)
    S = np.isin(lh, roots[sizes >= min_cells]) & Hs
    ll = lh if np.array_equal(Hs, Ls) else automask_ref.label(Ls)
    K = np.isin(ll, np.unique(ll[S])) & Ls
    return T_hi, T_lo, P, 0, ll, K


def sequential_sum(terms):
    """the terms added one by one in the order given (np.sum would add them pairwise)"""
    return float(np.add.accumulate(np.asarray(terms, dtype=np.float64))[-1])


def measure(image, cells, N):
    """The exact fields and the six sums of the island whose flat cell indices, ascending, are `cells` -> the first 15
    doubles of an info row, and per sum the sum of the absolute terms (what a bound on another summation order needs)."""
    v = image.ravel()[cells]
    y, x = cells // N, cells % N
    kp = int(cells[np.flatnonzero(v == v.max())[0]])  # (all values are > 0: the key order is the value order)
    yp, xp = kp // N, kp % N
    dx, dy = (x - xp).astype(np.float64), (y - yp).astype(np.float64)
    terms = [v, v * dx, v * dy, v * (dx * dx), v * (dx * dy), v * (dy * dy)]
    sums = [sequential_sum(t) for t in terms]
    mags = [float(np.abs(t).sum()) for t in terms]
    row = [float(cells[0]), float(cells.size), float(yp), float(xp), float(v.max()), *sums,
           float(y.min()), float(y.max()), float(x.min()), float(x.max())]
    return row, mags


def atan2_series(y, x):
    """atan2 from rounded +, -, *, / alone, step by step as the header states it: the same bits as the library's"""
    ax, ay = abs(x), abs(y)
    if ax == 0.0 and ay == 0.0:
        return 0.0
    swap = ay > ax
    t = ax / ay if swap else ay / ax
    base = 0.0
    if t > 0.4142135623730950488:
        t = (t - 1.0) / (t + 1.0)
        base = 0.25 * math.pi
    z = t * t
    s = 0.0
    for k in range(22, -1, -1):
        s = 1.0 / (2 * k + 1) - z * s
    r = base + t * s
    if swap:
        r = 0.5 * math.pi - r
    if x < 0.0:
        r = math.pi - r
    return 0.0 - r if y < 0.0 else r


def derive(row, T_lo, theta, N, border=0, beam=None, correct=True):
    """The component row and the flags of an island from the first 15 doubles of its info row, in the header's order.
    Also returns the intrinsic covariance (ixx, ixy, iyy) the shape was taken from (NaN with an unusable beam)."""
    yp, xp, Pi, S, Sx, Sy, Sxx, Sxy, Syy, y0, y1, x0, x1 = (float(t) for t in row[2:15])
    ox, oy = Sx / S, Sy / S
    cx, cy = xp + ox, yp + oy
    mxx, mxy, myy = Sxx / S - ox * ox, Sxy / S - ox * oy, Syy / S - oy * oy
    F = S
    if correct:
        t = T_lo / Pi
        if t > 0.0:
            u = 1.0 - t
            g = u / (1.0 - t * (1.0 - math.log(t)))
            F = F / u
            mxx, mxy, myy = mxx * g, mxy * g, myy * g
    flags = 0
    ixx, ixy, iyy = mxx, mxy, myy
    shaped = True
    if beam is not None:
        if beam_usable(beam):
            A, B, C = (float(beam[i]) for i in (0, 1, 2))
            det = A * C - B * B
            bxx, bxy, byy = beam_covariance(beam)
            F = F * math.sqrt(det) / math.pi
            ixx, ixy, iyy = mxx - bxx, mxy - bxy, myy - byy
        else:
            flags |= 4
            shaped = False
    bmaj = bmin = bpa = 0.0
    if not shaped:
        F = bmaj = bmin = bpa = math.nan
        ixx = ixy = iyy = math.nan
    else:
        d2 = ixx * iyy - ixy * ixy
        if ixx > 0.0 and iyy > 0.0 and d2 > 0.0:
            h, d = 0.5 * (ixx + iyy), 0.5 * (ixx - iyy)
            q = math.sqrt(d * d + ixy * ixy)
            lp = h + q
            lm = d2 / lp
            bmaj = math.sqrt(8.0 * LN2 * lp) * theta / N
            bmin = math.sqrt(8.0 * LN2 * lm) * theta / N
            bpa = 0.5 * math.pi - 0.5 * atan2_series(2.0 * ixy, ixx - iyy)
            if bpa > 0.5 * math.pi:
                bpa -= math.pi
        else:
            flags |= 1
    if y0 <= border or x0 <= border or y1 >= N - 1 - border or x1 >= N - 1 - border:
        flags |= 2
    half = float(N // 2)
    comp = [theta * (cx - half) / N, theta * (cy - half) / N, F, 0.0, 0.0, 0.0, bmaj, bmin, bpa, 0.0]
    return comp, flags, (ixx, ixy, iyy)


def pd_margin(cov):
    """How far the positive-definiteness test of step 4 is from flipping, relative to the sizes of its terms: the smallest
    of |ixx|, |iyy| over their sum and |ixx iyy - ixy^2| over ixx iyy + ixy^2."""
    ixx, ixy, iyy = cov
    tr, den = abs(ixx) + abs(iyy), abs(ixx * iyy) + ixy * ixy
    if tr == 0.0 or den == 0.0:
        return 0.0
    return min(abs(ixx) / tr, abs(iyy) / tr, abs(ixx * iyy - ixy * ixy) / den)


def shape_covariance(bmaj, bmin, bpa, theta, N):
    """the covariance (xx, xy, yy) in cells^2 of a component's (bmaj, bmin, bpa): the inverse of step 4"""
    c = 8.0 * LN2
    lp, lm = (bmaj * N / theta) ** 2 / c, (bmin * N / theta) ** 2 / c
    phi = 0.5 * math.pi - bpa
    cs, sn = math.cos(phi), math.sin(phi)
    return lp * cs * cs + lm * sn * sn, (lp - lm) * cs * sn, lp * sn * sn + lm * cs * cs


def find_sources(image, theta, sigma=None, border=0, thr=(0.0, 0.0), nsigma=(5.0, 2.5), peak_frac=0.0, min_cells=1,
                 beam=None, correct=True, max_c=None):
    """-> dict(comps (rows, 10), info (rows, 16), count, stats (8), mags (rows, 6), cov (rows, 3)); rows = min(count,
    max_c), max_c None: all.  sigma None stands for a NULL noise (both nsigma 0)."""
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    T_hi, T_lo, P, reason, ll, K = islands(image, sigma, border, thr, nsigma, peak_frac, min_cells)
    empty = dict(comps=np.zeros((0, COMP)), info=np.zeros((0, INFO)), count=0, mags=np.zeros((0, 6)), cov=np.zeros((0, 3)))
    if reason != 0:
        return dict(empty, stats=np.array([T_hi, T_lo, P, 0.0, 0.0, 0.0, 0.0, float(reason)]))
    inK = np.flatnonzero(K)  # ascending; a stable sort by label keeps every island's cells ascending
    order = np.argsort(ll.ravel()[inK], kind="stable")
    labels, sizes = np.unique(ll.ravel()[inK], return_counts=True)
    groups = np.split(inK[order], np.cumsum(sizes)[:-1]) if labels.size else []
    rows = labels.size if max_c is None else min(labels.size, int(max_c))
    comps, info, mags, covs = [], [], [], []
    for cells in groups[:rows]:
        row, mag = measure(image, cells, N)
        comp, flags, cov = derive(row, T_lo, theta, N, border, beam, correct)
        comps.append(comp)
        info.append(row + [float(flags)])
        mags.append(mag)
        covs.append(cov)
    comps = np.array(comps, dtype=np.float64).reshape(rows, COMP)
    flux = 0.0
    for f in comps[:, 2]:
        flux += float(f)
    points = float(np.count_nonzero((comps[:, 6] == 0.0) & (comps[:, 7] == 0.0)))
    stats = np.array([T_hi, T_lo, P, float(labels.size), float(rows), points, flux, 0.0])
    return dict(comps=comps, info=np.array(info, dtype=np.float64).reshape(rows, INFO), count=int(labels.size), stats=stats,
                mags=np.array(mags, dtype=np.float64).reshape(rows, 6), cov=np.array(covs, dtype=np.float64).reshape(rows, 3))
