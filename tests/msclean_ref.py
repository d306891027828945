"""Multi-scale CLEAN restated in numpy, statement by statement as include/gridhip.h ("multi-scale deconvolution") defines
it: the reference the msclean tests compare the library with.  The reference project has no deconvolution, so this
restatement is the only other implementation; tests/test_msclean_host.py checks it on a case worked by hand and against
tests/clean_ref.py for the delta scale alone.

numpy has no fused multiply-add, so the convolutions here round each product before adding it where the library fuses
the two: the set-up images agree to a few ulps of their magnitude, not bit for bit.  Everything else - the taps, the
scale choice, the products rounded before they are added or subtracted - is the header's arithmetic exactly, which is
why scales = [0] gives clean_ref's bits."""
import math

import numpy as np

import clean_ref


def default_bias(scales):
    """1 - 0.6 a_s / a_max, the binding's default (1 for the delta alone)"""
    a = np.asarray(scales, dtype=np.float64)
    return 1.0 - 0.6 * a / a.max() if a.max() > 0 else np.ones_like(a)


def scale_kernel(a):
    """m_s of the scale a > 0 as a (2 R + 1)^2 array [dy + R][dx + R], R = ceil(a) - 1; the delta ([[1.0]]) for a == 0"""
    if a == 0:
        return np.ones((1, 1))
    R = int(math.ceil(a)) - 1
    d = np.arange(-R, R + 1, dtype=np.float64)
    t = np.maximum(0.0, 1.0 - (d[None, :] * d[None, :] + d[:, None] * d[:, None]) / (a * a))
    rows = np.cumsum(t, axis=1)[:, -1]  # (cumsum adds in order from the first element: each row in dx order)
    total = np.cumsum(rows)[-1]         # (then the rows in dy order)
    return t / total


def convolve(m, X):
    """(m (*) X)[y, x] = sum of X[y - dy, x - dx] m(dy, dx), outside cells zero, the taps dy ascending then dx ascending
    from +0.0"""
    N = X.shape[0]
    R = m.shape[0] // 2
    pad = np.zeros((N + 2 * R, N + 2 * R))
    pad[R:R + N, R:R + N] = X
    acc = np.zeros((N, N))
    with np.errstate(invalid="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                acc += pad[R - dy:R - dy + N, R - dx:R - dx + N] * m[dy + R, dx + R]
    return acc


def setup(psf, scales):
    """(kernels m_s, cross-PSFs P[(s, t)] for s <= t, q_s): what depends on the PSF and the scale list alone"""
    S = len(scales)
    c = psf.shape[0] // 2
    m = [scale_kernel(a) for a in scales]
    P = {(0, 0): psf}
    for t in range(1, S):
        P[(0, t)] = convolve(m[t], psf)
    for t in range(1, S):
        for s in range(1, t + 1):
            P[(s, t)] = convolve(m[t], P[(0, s)])
    q = [float(P[(s, s)][c, c]) for s in range(S)]
    return m, P, q


def msclean(psf, residual, model, scales, bias, gain, threshold, niter, border=0, patch=0, trace=None, pre=None):
    """residual and model (N x N float64) are updated in place; returns the 12 stats.  trace, a list, receives per
    component (s*, k, gap), gap the relative distance between the two largest |b_s (R_s / q_s)| over all searched cells of
    all scales.  pre: setup(psf, scales) computed earlier (it does not depend on the residual)."""
    N = residual.shape[0]
    c = N // 2
    S = len(scales)
    m, P, q = pre if pre is not None else setup(psf, scales)
    R = [residual] + [convolve(m[t], residual) for t in range(1, S)]
    iters, flux, last, n = 0, 0.0, -1, [0] * 6

    def stats(p0, k0):
        return np.array([iters, p0, float(k0), float(last), flux, 0.0, *map(float, n)])

    while True:
        ks = [clean_ref.peak(R[s], border)[0] for s in range(S)]
        k0 = ks[0]
        if k0 < 0:
            return stats(np.nan, -1)
        p0 = R[0].flat[k0]
        if iters >= niter or abs(p0) <= threshold:
            return stats(p0, k0)
        best, top = -1, 0.0
        with np.errstate(all="ignore"):
            for s in range(S):
                if ks[s] < 0 or not (q[s] > 0.0 and q[s] < math.inf):
                    continue
                v = abs(bias[s] * (R[s].flat[ks[s]] / q[s]))
                if best < 0 or v > top:
                    best, top = s, v
        if best < 0:
            return stats(p0, k0)
        k = ks[best]
        y, x = divmod(k, N)
        if trace is not None:
            vals = []
            with np.errstate(all="ignore"):
                for s in range(S):
                    if ks[s] < 0 or not (q[s] > 0.0 and q[s] < math.inf):
                        continue
                    a = np.abs(bias[s] * (R[s][border:N - border, border:N - border] / q[s])).ravel()
                    a = a[~np.isnan(a)]
                    vals.append(np.partition(a, -2)[-2:] if a.size > 1 else a)
            two = np.sort(np.concatenate(vals))[-2:]
            trace.append((best, k, (two[-1] - two[0]) / two[-1] if two.size > 1 else 1.0))
        f = gain * (R[best].flat[k] / q[best])
        flux += f
        n[best] += 1
        last = best
        # the model blob: f * m_s* over the kernel's support, clipped to the image (the product rounded, then added)
        r = m[best].shape[0] // 2
        ylo, yhi, xlo, xhi = max(0, y - r), min(N - 1, y + r), max(0, x - r), min(N - 1, x + r)
        model[ylo:yhi + 1, xlo:xhi + 1] += f * m[best][ylo - y + r:yhi - y + r + 1, xlo - x + r:xhi - x + r + 1]
        # every R_t loses f * P_{s* t}, shifted to the component: Hogbom's clipping and patch rule
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        for t in range(S):
            Pst = P[(min(best, t), max(best, t))]
            R[t][ylo:yhi + 1, xlo:xhi + 1] -= f * Pst[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
        iters += 1


def extended_sky(psf, seed, noise=1e-3):
    """(dirty image, true flux): one sigma = 4 Gaussian - centred left of the middle column so that at N = 200 it
    straddles column 128, the boundary of two tile columns - plus two point sources of opposite sign, convolved with the
    PSF (circularly, through the transform), plus Gaussian noise"""
    N = psf.shape[0]
    c = N // 2
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:N, 0:N]
    gy, gx = c + 3, (128 if N >= 160 else c - 5)
    sky = np.exp(-0.5 * ((yy - gy) ** 2 + (xx - gx) ** 2) / 16.0)
    sky[c - N // 5, c + N // 6] += 2.0
    sky[c + N // 4, c - N // 5] -= 1.5
    shift = np.roll(np.roll(psf, -c, axis=0), -c, axis=1)
    img = np.fft.ifft2(np.fft.fft2(sky) * np.fft.fft2(shift)).real
    img += noise * rng.normal(size=(N, N))
    return np.ascontiguousarray(img), float(sky.sum())
