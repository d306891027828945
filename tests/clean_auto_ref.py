"""The _auto forms of clean and msclean restated in numpy, statement by statement as include/gridhip.h ("masks and
noise-based stop levels") defines them on top of tests/clean_ref.py and tests/msclean_ref.py: a mask in the search, the
stop level T = max(threshold, nsigma * sigma, peak_frac * |first peak|) and the reason codes."""
import math
from fractions import Fraction

import numpy as np

import clean_ref
import msclean_ref


def masked(residual, mask):
    """the residual as the search sees it: a cell the mask leaves out is skipped exactly as a NaN cell is"""
    return residual if mask is None else np.where(np.asarray(mask) != 0, residual, np.nan)


def stop_level(threshold, nsigma, sigma, peak_frac, p1):
    """(T, bad): each product rounded once; a term whose factor is 0 is left out, and so is the peak's when there is
    none; bad: nsigma > 0 and sigma is NaN"""
    T = float(threshold)
    if nsigma > 0:
        if sigma != sigma:
            return math.nan, True
        T = max(T, nsigma * sigma)
    if peak_frac > 0 and p1 == p1:
        T = max(T, peak_frac * abs(p1))
    return T, False


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the nearest double)"""
    if not all(map(math.isfinite, (a, b, c))):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def clean(psf, residual, model, gain, threshold, niter, border=0, patch=0, mask=None, nsigma=0.0, sigma=None,
          peak_frac=0.0, trace=None):
    """residual and model are updated in place; returns the 8 stats [iterations, final peak, its flat index, flux, T,
    reason, first peak, 0].  trace, a list, receives per peak looked at - the stopping one included - (k, |peak|, the
    relative gap between the two largest |residual| under the mask)."""
    N = residual.shape[0]
    c = N // 2
    iters, flux = 0, 0.0
    T = p1 = None
    while True:
        k, second = clean_ref.peak(masked(residual, mask), border)
        p = residual.flat[k] if k >= 0 else math.nan
        if T is None:
            p1 = p
            T, bad = stop_level(threshold, nsigma, sigma, peak_frac, p1)
            if bad:
                return np.array([0.0, p, float(k), 0.0, T, 3.0, p1, 0.0])
        if k < 0:
            return np.array([iters, math.nan, -1.0, flux, T, 2.0, p1, 0.0])
        if trace is not None:
            trace.append((k, abs(p), (abs(p) - second) / abs(p) if abs(p) > 0 else 1.0))
        if abs(p) <= T:
            return np.array([iters, p, float(k), flux, T, 1.0, p1, 0.0])
        if iters >= niter:
            return np.array([iters, p, float(k), flux, T, 0.0, p1, 0.0])
        y, x = divmod(k, N)
        f = gain * p  # (rounded once: what the PSF is scaled by)
        # the model cell and the flux receive gain * p in one fused step each, as gridhip_clean's pick kernel adds them
        # (include/gridhip.h says so of the model under "multi-scale deconvolution"); tests/clean_ref.py rounds the
        # product first, which differs in the last bit and is why the plain tests allow 1e-10
        model[y, x] = fma(gain, p, model[y, x])
        flux = fma(gain, p, flux)
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        residual[ylo:yhi + 1, xlo:xhi + 1] -= f * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
        iters += 1


def msclean(psf, residual, model, scales, bias, gain, threshold, niter, border=0, patch=0, mask=None, nsigma=0.0,
            sigma=None, peak_frac=0.0, trace=None, pre=None):
    """msclean_ref.msclean with the mask in the search of every scale, the stop level and the reason: returns the 16
    stats.  trace receives per component (s*, k, |p_0|); the stopping peak is appended as (-1, k_0, |p_0|)."""
    N = residual.shape[0]
    c = N // 2
    S = len(scales)
    m, P, q = pre if pre is not None else msclean_ref.setup(psf, scales)
    R = [residual] + [msclean_ref.convolve(m[t], residual) for t in range(1, S)]
    iters, flux, last, n = 0, 0.0, -1, [0] * 6
    T = p1 = None

    def stats(p0, k0, reason):
        return np.array([iters, p0, float(k0), float(last), flux, 0.0, *map(float, n), T, float(reason), p1, 0.0])

    while True:
        ks = [clean_ref.peak(masked(R[s], mask), border)[0] for s in range(S)]
        k0 = ks[0]
        p0 = R[0].flat[k0] if k0 >= 0 else math.nan
        if T is None:
            p1 = p0
            T, bad = stop_level(threshold, nsigma, sigma, peak_frac, p1)
            if bad:
                return stats(p0, k0, 3)
        if k0 < 0:
            return stats(math.nan, -1, 2)
        if abs(p0) <= T or iters >= niter:
            if trace is not None:
                trace.append((-1, k0, abs(p0)))
            return stats(p0, k0, 1 if abs(p0) <= T else 0)
        best, top = -1, 0.0
        with np.errstate(all="ignore"):
            for s in range(S):
                if ks[s] < 0 or not (q[s] > 0.0 and q[s] < math.inf):
                    continue
                v = abs(bias[s] * (R[s].flat[ks[s]] / q[s]))
                if best < 0 or v > top:
                    best, top = s, v
        if best < 0:
            return stats(p0, k0, 2)
        k = ks[best]
        y, x = divmod(k, N)
        if trace is not None:
            trace.append((best, k, abs(p0)))
        r = R[best].flat[k] / q[best]
        f = gain * r
        flux += f
        n[best] += 1
        last = best
        if best == 0:  # (the delta's one cell receives gain * (p / q) in one fused step)
            model[y, x] = fma(gain, r, model[y, x])
        else:
            h = m[best].shape[0] // 2
            ylo, yhi, xlo, xhi = max(0, y - h), min(N - 1, y + h), max(0, x - h), min(N - 1, x + h)
            model[ylo:yhi + 1, xlo:xhi + 1] += f * m[best][ylo - y + h:yhi - y + h + 1, xlo - x + h:xhi - x + h + 1]
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        for t in range(S):
            Pst = P[(min(best, t), max(best, t))]
            R[t][ylo:yhi + 1, xlo:xhi + 1] -= f * Pst[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
        iters += 1
