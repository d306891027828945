"""The numpy restatement of gridhip_mosaic / gridhip_reproject (include/gridhip.h, "reprojection and mosaicking"): one
rounded operation per numpy operation, in the order of the header's rule, so that the device's bits can be compared with
`==`.  numpy rounds every elementwise product, sum, quotient, sqrt and floor to nearest, as fp64 on the device does with
contraction off; nothing here uses a fused multiply-add, a dot product or a sum over an axis."""
import numpy as np

f64 = np.float64
KINDS = {"nearest": 0, "bilinear": 1, "cubic": 3}


def rotation_ok(r):
    """phase_shift's rule for one R (9 values): finite, R22 > 0, every entry of |R R^T - I| <= 1e-9"""
    r = np.asarray(r, dtype=f64).ravel()
    if not np.isfinite(r).all() or not r[8] > 0.0:
        return False
    for i in range(3):
        for j in range(3):
            d = r[3 * i] * r[3 * j] + r[3 * i + 1] * r[3 * j + 1] + r[3 * i + 2] * r[3 * j + 2] - (1.0 if i == j else 0.0)
            if not abs(d) <= 1e-9:
                return False
    return True


def cell_coords(N, theta):
    """l of the cells x = 0 .. N-1: theta (x - N/2) / N, the product first"""
    return f64(theta) * (np.arange(N) - N // 2).astype(f64) / f64(N)


def feather(d, inner, outer):
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (outer - d) / (outer - inner)
        s = (t * t) * (3.0 - 2.0 * t)
    return np.where(d <= inner, 1.0, np.where(d >= outer, 0.0, s))


def keys(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
            ((0.5 * t - 0.5) * t) * t]


def _index(fx, lo, hi):
    """floor(fx) as integers where lo <= floor(fx) <= hi (judged on the doubles: inf and NaN are outside), lo elsewhere"""
    i = np.floor(fx)
    ok = (i >= lo) & (i <= hi)
    return np.where(ok, i, lo).astype(np.int64), ok


def bilinear(img, fx, fy):
    """(sample, footprint inside, all four taps finite)"""
    Ns = img.shape[0]
    if Ns < 2:
        z = np.zeros(fx.shape)
        return z, np.zeros(fx.shape, dtype=bool), np.zeros(fx.shape, dtype=bool)
    ix, okx = _index(fx, 0, Ns - 2)
    iy, oky = _index(fy, 0, Ns - 2)
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty = fx - ix, fy - iy
        a, b, c, d = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
        r0 = a * (1.0 - tx) + b * tx
        r1 = c * (1.0 - tx) + d * tx
        v = r0 * (1.0 - ty) + r1 * ty
    return v, okx & oky, np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d)


def sample(img, fx, fy, kind):
    """(sample, footprint inside, all taps finite) of step 5"""
    Ns = img.shape[0]
    if kind == 0:
        with np.errstate(invalid="ignore"):
            ix, okx = _index(0.5 + fx, 0, Ns - 1)
            iy, oky = _index(0.5 + fy, 0, Ns - 1)
        v = img[iy, ix]
        return v, okx & oky, np.isfinite(v)
    if kind == 1:
        return bilinear(img, fx, fy)
    if Ns < 4:
        z = np.zeros(fx.shape)
        return z, np.zeros(fx.shape, dtype=bool), np.zeros(fx.shape, dtype=bool)
    ix, okx = _index(fx, 1, Ns - 3)
    iy, oky = _index(fy, 1, Ns - 3)
    fin = np.ones(fx.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        cx, cy = keys(fx - ix), keys(fy - iy)
        rows = []
        for j in range(4):
            a, b, c, d = (img[iy + j - 1, ix + k - 1] for k in range(4))
            fin &= np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d)
            rows.append(((cx[0] * a + cx[1] * b) + cx[2] * c) + cx[3] * d)
        v = ((cy[0] * rows[0] + cy[1] * rows[1]) + cy[2] * rows[2]) + cy[3] * rows[3]
    return v, okx & oky, fin


def mosaic(facets, theta_s, R, theta_d, Nd, kind="cubic", weights=None, window=None, normalize=True, wmin=0.0,
           blank=np.nan):
    """(out, wsum, stats) by the header's rule.  facets (F, Ns, Ns); R (F, 9) or (F, 3, 3); window (inner, outer) in cells,
    None for inner = outer = Ns / 2."""
    facets = np.asarray(facets, dtype=f64)
    if facets.ndim == 2:
        facets = facets[None]
    F, Ns = facets.shape[0], facets.shape[1]
    R = np.asarray(R, dtype=f64).reshape(F, 9)
    kind = KINDS.get(kind, kind)
    inner, outer = (Ns / 2, Ns / 2) if window is None else (float(window[0]), float(window[1]))
    theta_s, h = f64(theta_s), f64(Ns // 2)
    lc = cell_coords(Nd, theta_d)
    l, m = np.meshgrid(lc, lc)  # l varies along x (columns), m along y (rows)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = l * l + m * m
        live = r2 < 1.0
        n = np.sqrt(np.where(live, 1.0 - r2, 0.0))
    num, den = np.zeros((Nd, Nd)), np.zeros((Nd, Nd))
    cnt = np.zeros((Nd, Nd), dtype=np.int64)
    left, used = 0, 0
    for f in range(F):
        r = R[f]
        if not rotation_ok(r):
            continue
        used += 1
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            npr = (r[6] * l + r[7] * m) + r[8] * n
            cover = live & (npr > 0.0)
            lp = (r[0] * l + r[1] * m) + r[2] * n
            mp = (r[3] * l + r[4] * m) + r[5] * n
            fx = (lp * f64(Ns)) / theta_s + h
            fy = (mp * f64(Ns)) / theta_s + h
            w = feather(np.abs(fx - h), inner, outer) * feather(np.abs(fy - h), inner, outer)
            cover &= ~(w == 0.0)
            v, ins, fin = sample(facets[f], fx, fy, kind)
            cover &= ins
            left += int((cover & ~fin).sum())
            cover &= fin
            if weights is not None:
                q, qin, _ = bilinear(np.asarray(weights, dtype=f64).reshape(facets.shape)[f], fx, fy)
                cover &= qin
                cover &= np.isfinite(q) & (q > 0.0)
                w = w * q
            num = np.where(cover, num + w * v, num)
            den = np.where(cover, den + w, den)
        cnt += cover
    covered = live & (den > wmin)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out = np.where(covered, num / den if normalize else num, blank)
    wsum = np.where(covered, den, 0.0)
    ncov = int(covered.sum())
    stats = np.array([ncov, Nd * Nd - ncov, used, F - used, left, int(cnt.max()) if cnt.size else 0, 0, 0], dtype=f64)
    return out, wsum, stats


def reproject(image, theta_s, R, theta_d, Nd, kind="cubic", window=None, blank=np.nan):
    return mosaic(np.asarray(image)[None], theta_s, np.asarray(R).reshape(1, 9), theta_d, Nd, kind, None, window, True, 0.0,
                  blank)[0]


def same_bits(a, b):
    """equal as bit patterns, NaN payloads and signed zeros included"""
    a, b = np.ascontiguousarray(a, dtype=f64), np.ascontiguousarray(b, dtype=f64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
