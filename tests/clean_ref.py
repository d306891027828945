"""Hogbom CLEAN restated in numpy, statement by statement as include/gridhip.h ("deconvolution") defines it: the
reference the clean tests compare the library with.  The reference project has no deconvolution, so this restatement is
the only other implementation; tests/test_clean_host.py checks it on a case computed by hand."""
import numpy as np


def peak(residual, border):
    """(k, second): the flat index of the largest |residual| over border <= y, x < N - border - ties to the lowest flat
    index, NaN never - or -1 when every searched cell is NaN; and the second largest magnitude there (-1 when none)"""
    N = residual.shape[0]
    a = np.abs(residual[border:N - border, border:N - border])
    a = np.where(np.isnan(a), -1.0, a)
    j = int(np.argmax(a))  # the first of equal maxima in row-major order: the lowest flat index
    if a.flat[j] < 0:
        return -1, -1.0
    y, x = divmod(j, a.shape[1])
    second = np.partition(a.ravel(), -2)[-2] if a.size > 1 else -1.0
    return (y + border) * N + x + border, float(second)


def clean(psf, residual, model, gain, threshold, niter, border=0, patch=0, trace=None):
    """residual and model (N x N float64) are updated in place; returns stats = [iterations, final peak, its flat index,
    flux].  trace, a list, receives per component (k, the relative gap between the two largest |residual|)."""
    N = residual.shape[0]
    c = N // 2
    iters, flux = 0, 0.0
    while True:
        k, second = peak(residual, border)
        if k < 0:
            return np.array([iters, np.nan, -1.0, flux])
        y, x = divmod(k, N)
        p = residual[y, x]
        if iters >= niter or abs(p) <= threshold:
            return np.array([iters, p, float(k), flux])
        if trace is not None:
            trace.append((k, (abs(p) - second) / abs(p)))
        f = gain * p
        model[y, x] += f
        flux += f
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        # (the product is rounded, then subtracted: numpy does not fuse the two)
        residual[ylo:yhi + 1, xlo:xhi + 1] -= f * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
        iters += 1


def make_psf(N, seed, fill=0.04):
    """A PSF as an imager makes it: random uv coverage, made point-symmetric about the centre cell so that the PSF is
    real, through the centred inverse transform, normalised to 1 at its zero-lag cell (N // 2, N // 2)."""
    rng = np.random.default_rng(seed)
    c = N // 2
    yy, xx = np.mgrid[0:N, 0:N]
    r2 = ((yy - c) ** 2 + (xx - c) ** 2) / float(c * c)
    w = (rng.random((N, N)) < fill * np.exp(-2.0 * r2)).astype(np.float64)
    idx = (2 * c - np.arange(N)) % N
    w = w + w[idx][:, idx]
    psf = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(w))).real
    psf = psf / psf[c, c]
    assert np.argmax(psf) == c * N + c
    return np.ascontiguousarray(psf)


def make_sky(psf, seed, nsrc=25, noise=1e-3):
    """(dirty image, source list): nsrc point sources of both signs in the inner half convolved with the PSF (the
    clipped shift clean itself subtracts) plus Gaussian noise"""
    N = psf.shape[0]
    c = N // 2
    rng = np.random.default_rng(seed)
    ys, xs = rng.integers(N // 4, N - N // 4, nsrc), rng.integers(N // 4, N - N // 4, nsrc)
    amp = rng.uniform(0.2, 1.0, nsrc) * rng.choice([-1.0, 1.0], nsrc)
    img = np.zeros((N, N))
    for y, x, a in zip(ys, xs, amp):
        ylo, yhi, xlo, xhi = max(0, y - c), min(N - 1, y - c + N - 1), max(0, x - c), min(N - 1, x - c + N - 1)
        img[ylo:yhi + 1, xlo:xhi + 1] += a * psf[ylo - y + c:yhi - y + c + 1, xlo - x + c:xhi - x + c + 1]
    img += noise * rng.normal(size=(N, N))
    return img, list(zip(ys, xs, amp))
