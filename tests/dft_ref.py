"""numpy restatement of gridhip_dft_predict and gridhip_components_from_image (include/gridhip.h, "direct-Fourier
prediction"): the definition the GPU tests compare against.  The phase is evaluated in np.longdouble, so the reference's
own error at |p| ~ 1e4 turns is far below the 1e-10 sum |S| the tests allow."""
import numpy as np

COMP_DOUBLES = 10
TOL = 1e-10  # |vis - ref| <= TOL * sum_c |S_c|: three roundings of p at |p| <= 1e4 turns cost 2 pi 3 1e4 2^-53 ~ 2e-11


def pixel_lm(theta, N, x, y):
    """the direction cosines of pixel [y][x] of an N x N image of field of view theta"""
    return theta * (np.asarray(x) - N // 2) / N, theta * (np.asarray(y) - N // 2) / N


def skipped(comps, T):
    """which rows are SKIPPED: a read field that is not finite, r2 > 1, bmaj < bmin, bmin < 0, or a bmaj whose square
    overflows (the quadratic form of the Gaussian is then not finite)"""
    c = np.asarray(comps, dtype=np.float64).reshape(-1, COMP_DOUBLES)
    read = np.concatenate([c[:, :2 + T], c[:, 6:9]], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]
        form = (np.pi ** 2 / (4 * np.log(2))) * c[:, 6] * c[:, 6]  # (the largest coefficient of the Gaussian's form)
        return (~np.isfinite(read).all(axis=1) | (r2 > 1.0) | (c[:, 6] < c[:, 7]) | (c[:, 7] < 0.0) | ~np.isfinite(form))


def flux(comps, T, x):
    """S_c(x_k), shape (n, C): Horner with every product rounded; only f0 .. f_{T-1} are read"""
    c = np.asarray(comps, dtype=np.float64).reshape(-1, COMP_DOUBLES)
    x = np.asarray(x, dtype=np.float64)[:, None]
    s = np.broadcast_to(c[None, :, 2 + T - 1], (x.shape[0], c.shape[0])).copy()
    for t in range(T - 2, -1, -1):
        s = c[None, :, 2 + t] + x * s
    return s


def dft_predict(comps, u, v, w=None, x=None, T=1, count=None, vis_sub=None, wsign=1.0):
    """-> (vis_out, stats[:3]) as gridhip_dft_predict defines them; wsign = -1 evaluates the WRONG sign of w (test 11)"""
    c = np.asarray(comps, dtype=np.float64).reshape(-1, COMP_DOUBLES)
    C = c.shape[0] if count is None else min(max(int(count), 0), c.shape[0])
    c = c[:C]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = u.shape[0]
    w = np.zeros(n) if w is None else np.asarray(w, dtype=np.float64)
    xs = np.zeros(n) if x is None else np.asarray(x, dtype=np.float64)
    bad = ~(np.isfinite(u) & np.isfinite(v) & np.isfinite(w) & np.isfinite(xs))
    skip = skipped(c, T)
    good = c[~skip]
    uu, vv, ww, xx = (np.where(bad, 0.0, a) for a in (u, v, w, xs))
    L = np.longdouble
    l, m = good[:, 0].astype(L), good[:, 1].astype(L)
    r2 = l * l + m * m
    nm1 = -r2 / (1 + np.sqrt(1 - r2))
    p = uu.astype(L)[:, None] * l[None, :] + vv.astype(L)[:, None] * m[None, :] + wsign * ww.astype(L)[:, None] * nm1[None, :]
    r = p - np.rint(p)
    ang = 2 * np.arctan2(L(0), L(-1)) * r  # (pi to longdouble precision)
    S = flux(good, T if x is not None else 1, xx)
    bmaj, bmin, bpa = good[:, 6], good[:, 7], good[:, 8]
    up = uu[:, None] * np.sin(bpa)[None, :] + vv[:, None] * np.cos(bpa)[None, :]
    vp = uu[:, None] * np.cos(bpa)[None, :] - vv[:, None] * np.sin(bpa)[None, :]
    E = np.exp(-(np.pi ** 2 / (4 * np.log(2))) * (bmaj[None, :] ** 2 * up ** 2 + bmin[None, :] ** 2 * vp ** 2))
    E = np.where(((bmaj == 0) & (bmin == 0))[None, :], 1.0, E)
    amp = (S * E).astype(L)
    pred = ((amp * np.cos(ang)).sum(axis=1).astype(np.float64) - 1j * (amp * np.sin(ang)).sum(axis=1).astype(np.float64))
    pred = np.where(bad, 0.0, pred)
    out = pred if vis_sub is None else np.asarray(vis_sub, dtype=np.complex128) - pred
    return out, np.array([C - skip.sum(), skip.sum(), bad.sum()], dtype=np.float64)


def flux_scale(comps, T, x=None, n=1):
    """sum_c |S_c(x_k)| per visibility over the components that are not skipped: what TOL multiplies"""
    c = np.asarray(comps, dtype=np.float64).reshape(-1, COMP_DOUBLES)
    good = c[~skipped(c, T)]
    xs = np.zeros(n) if x is None else np.where(np.isfinite(x), x, 0.0)
    return np.abs(flux(good, T if x is not None else 1, xs)).sum(axis=1)


def components_from_image(theta, model):
    """-> the full list (found, 10) of a (T, N, N) or (N, N) model, row-major"""
    m = np.asarray(model, dtype=np.float64)
    m = m[None] if m.ndim == 2 else m
    T, N, _ = m.shape
    y, x = np.nonzero((m != 0).any(axis=0))  # (row-major; NaN != 0)
    out = np.zeros((len(y), COMP_DOUBLES))
    out[:, 0], out[:, 1] = pixel_lm(theta, N, x, y)
    out[:, 2:2 + T] = m[:, y, x].T
    return out


def selfcal_observation():
    """The end-to-end case of tests/test_gpu_dft.py and tests/test_dft_host.py: three point sources off pixel centres in a
    64 x 64 field, 8 antennas, all 28 baselines at 4 times (w = 0) -> theta, lam, N, A, u, v, a1, a2, comps, the sources
    pixelised to their nearest cells, and the true gains [1][A]."""
    rng = np.random.default_rng(2026)
    theta, lam, N, A, times = 0.1, 640, 64, 8, 4
    pos = rng.uniform(-140, 140, (A, 2))  # wavelengths: every baseline stays inside the grid
    p, q = np.triu_indices(A, 1)
    us, vs = [], []
    for t in range(times):
        ang = 0.35 * t
        b = (pos[p] - pos[q]) @ np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]).T
        us.append(b[:, 0])
        vs.append(b[:, 1])
    u, v = np.concatenate(us), np.concatenate(vs)
    a1, a2 = np.tile(p, times).astype(np.int64), np.tile(q, times).astype(np.int64)
    px = np.array([[40.3, 28.6], [20.7, 45.4], [33.5, 31.5]])  # (x, y) in cells
    fl = np.array([3.0, 2.0, 1.0])
    comps = np.zeros((3, COMP_DOUBLES))
    comps[:, 0], comps[:, 1] = pixel_lm(theta, N, px[:, 0], px[:, 1])
    comps[:, 2] = fl
    model = np.zeros((N, N))
    for (x, y), f in zip(px, fl):
        model[int(np.floor(y + 0.5)), int(np.floor(x + 0.5))] += f
    gt = (1 + 0.2 * rng.normal(size=(1, A))) * np.exp(1j * rng.uniform(-1, 1, (1, A)))
    return theta, lam, N, A, u, v, a1, a2, comps, model, gt


# chi^2 of the solve (niter 200, tol 1e-7) against the exact model and against the nearest-cell prediction of the
# pixelised sources, from gaincal_ref on this file's model: 4.168e-11 and 341.1, ratio 1.222e-13; asserted with a 10x margin
SELFCAL_SOLVE = dict(niter=200, tol=1e-7)
SELFCAL_RATIO = 10 * 1.222e-13
