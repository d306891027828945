"""Joint CLEAN restated in numpy, statement by statement as include/gridhip.h ("joint deconvolution") defines it, on top
of clean_ref.peak (the search rule) and clean_auto_ref.masked / fma (the mask in the search, the fused model step): the
reference the jclean tests compare the library with.  The reference project has no deconvolution, so this restatement is
the only other implementation; tests/test_jclean_host.py checks it on a case computed by hand and, for one plane, against
the Hogbom restatement with a stop level (tests/clean_auto_ref.py)."""
import functools
import math

import numpy as np

import clean_auto_ref
import clean_ref

METRICS = {"sum": 0, "sumsq": 1}


def power(x, metric):
    """x^d, d = metric + 1: x itself, or x * x rounded once"""
    return x if metric == 0 else x * x


def statistic(residuals, weights, metric):
    """s = w_0 * R_0^d + w_1 * R_1^d + ..., p ascending from the first term, every product rounded, then added"""
    s = weights[0] * power(residuals[0], metric)
    for p in range(1, len(residuals)):
        s = s + weights[p] * power(residuals[p], metric)
    return s


def stop_level(threshold, nsigma, sigma, peak_frac, s1, metric):
    """(L, bad): L = max(threshold^d, (nsigma * sigma)^d, peak_frac^d * |s1|), every product rounded once; a term whose
    factor is 0 is left out, and so is s1's when there is none; bad: nsigma > 0 and sigma is NaN"""
    L = power(threshold, metric)
    if nsigma > 0:
        if sigma != sigma:
            return math.nan, True
        L = max(L, power(nsigma * sigma, metric))
    if peak_frac > 0 and s1 == s1:
        L = max(L, power(peak_frac, metric) * abs(s1))
    return L, False


def jclean(psfs, residuals, models, weights=None, metric=1, gain=0.1, threshold=0.0, niter=100, border=0, patch=0,
           mask=None, nsigma=0.0, sigma=None, peak_frac=0.0, trace=None, fma=clean_auto_ref.fma):
    """psfs [Q, N, N], Q in (1, P); residuals and models [P, N, N], updated in place; weights: P numbers, None: all 1.
    Returns the 16 stats [iterations, s at the final peak, its flat index, L, reason, first s, 0, 0, flux_0 .. flux_7].
    trace, a list, receives per component (k, the relative gap between the two largest |s| under the mask).  fma: the
    fused step of the models and the flux (clean_auto_ref's takes Python floats; a run in another dtype, where the
    fixture makes every operation exact anyway, passes a plain one)."""
    P, N = residuals.shape[0], residuals.shape[1]
    Q = psfs.shape[0]
    assert Q in (1, P) and psfs.shape[1:] == (N, N) and models.shape == residuals.shape and 1 <= P <= 8
    dt = residuals.dtype.type
    w = [dt(1.0)] * P if weights is None else [dt(v) for v in weights]
    gain, threshold = dt(gain), dt(threshold)
    c = N // 2
    iters, flux = 0, [dt(0.0)] * 8
    L = s1 = None

    def stats(sk, k, reason):
        return np.array([iters, sk, float(k), L, float(reason), s1, 0.0, 0.0] + flux, dtype=residuals.dtype)

    while True:
        with np.errstate(invalid="ignore", over="ignore"):
            s = statistic(residuals, w, metric)
        k, second = clean_ref.peak(clean_auto_ref.masked(s, mask), border)
        sk = s.flat[k] if k >= 0 else dt(math.nan)
        if L is None:
            s1 = sk
            L, bad = stop_level(threshold, dt(nsigma), None if sigma is None else dt(sigma), dt(peak_frac), s1, metric)
            if bad:
                return stats(sk, k, 3)
        if k < 0:
            return stats(dt(math.nan), -1, 2)
        if abs(sk) <= L:  # (before anything is subtracted, and before the niter test)
            return stats(sk, k, 1)
        if iters >= niter:
            return stats(sk, k, 0)
        if trace is not None:
            trace.append((k, float((abs(sk) - second) / abs(sk))))
        y, x = divmod(k, N)
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        for p in range(P):
            R = residuals[p][y, x]
            f = gain * R  # (rounded once: what the PSF is scaled by)
            models[p][y, x] = fma(gain, R, models[p][y, x])
            flux[p] = fma(gain, R, flux[p])
            psf = psfs[p if Q == P else 0]
            # (the product is rounded, then subtracted: numpy does not fuse the two)
            residuals[p][ylo:yhi + 1, xlo:xhi + 1] -= f * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
        iters += 1


def default_weights(metric, P):
    """what Context.jclean passes for weights=None: the mean image for "sum", 1 each for "sumsq" """
    return [1.0 / P] * P if metric == "sum" else [1.0] * P


@functools.lru_cache(maxsize=None)
def make_psfs(N, Q):
    """psfs[p] = clean_ref.make_psf(N, 300 + p): shared between the tests, never written to"""
    out = np.stack([clean_ref.make_psf(N, 300 + p) for p in range(Q)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_sky(N, P, Q, nsrc=12, noise=1e-3):
    """The P dirty images of one sky: nsrc point sources at shared positions in the inner half, per-plane amplitudes
    0.2 .. 1 - signed for a shared PSF (Stokes planes), positive for per-plane PSFs (channels) - each laid in through its
    plane's PSF (the clipped shift the clean itself subtracts), plus Gaussian noise in every plane"""
    psfs = make_psfs(N, Q)
    c = N // 2
    rng = np.random.default_rng(400)
    ys, xs = rng.integers(N // 4, N - N // 4, nsrc), rng.integers(N // 4, N - N // 4, nsrc)
    amp = rng.uniform(0.2, 1.0, (P, nsrc))
    if Q == 1:
        amp = amp * rng.choice([-1.0, 1.0], (P, nsrc))
    img = np.zeros((P, N, N))
    for p in range(P):
        psf = psfs[p if Q == P else 0]
        for y, x, a in zip(ys, xs, amp[p]):
            ylo, yhi, xlo, xhi = max(0, y - c), min(N - 1, y - c + N - 1), max(0, x - c), min(N - 1, x - c + N - 1)
            img[p, ylo:yhi + 1, xlo:xhi + 1] += a * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
    img += noise * rng.normal(size=(P, N, N))
    img.setflags(write=False)
    return img


def midway_threshold(psfs, img, weights, metric, border=0, patch=0):
    """A threshold, in image units, that a clean of img reaches after some components and before many: half the first
    peak - 0.5 * |s1| for "sum", 0.5 * sqrt(s1) for "sumsq" - from a run with niter = 0"""
    s1 = jclean(psfs, img.copy(), np.zeros_like(img), weights, metric, 1.0, 0.0, 0, border, patch)[5]
    return 0.5 * abs(s1) if metric == 0 else 0.5 * math.sqrt(s1)
