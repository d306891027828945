"""Multi-term CLEAN restated in numpy, statement by statement as include/gridhip.h ("wide-band imaging") defines it: the
reference the mfclean tests compare the library with.  The reference project has no deconvolution, so this restatement is
the only other implementation; tests/test_mfclean_host.py checks it on a case computed by hand and, for one term, against
the Hogbom restatement (tests/clean_ref.py).  The one place it does not restate the library's bits: models[t][k] += f_t and
flux_t += f_t are a rounded product and a sum here, one fused step on the device (the header's note on rounding)."""
import numpy as np

import clean_ref


def invert(H):
    """(Hinv, ok): Gauss-Jordan without pivoting in Python floats, rows in order - the pivot row divided by the pivot,
    then m * (pivot row) taken from every other row, the product rounded, then subtracted.  ok is False when a pivot is
    not > 0 (NaN included)."""
    T = len(H)
    A = [[float(H[t][q]) for q in range(T)] for t in range(T)]
    B = [[1.0 if t == q else 0.0 for q in range(T)] for t in range(T)]
    for i in range(T):
        piv = A[i][i]
        if not piv > 0.0:
            return None, False
        A[i] = [v / piv for v in A[i]]
        B[i] = [v / piv for v in B[i]]
        for r in range(T):
            if r == i:
                continue
            m = A[r][i]
            A[r] = [A[r][j] - m * A[i][j] for j in range(T)]
            B[r] = [B[r][j] - m * B[i][j] for j in range(T)]
    return B, True


def coefficients(Hinv, R):
    """a[t] = sum_q Hinv[t][q] * R[q], q ascending from the first product, each product rounded, then added"""
    T = len(Hinv)
    a = []
    for t in range(T):
        s = Hinv[t][0] * R[0]
        for q in range(1, T):
            s = s + Hinv[t][q] * R[q]
        a.append(s)
    return a


def score(a, R):
    s = a[0] * R[0]
    for t in range(1, len(a)):
        s = s + a[t] * R[t]
    return s


def mfclean(psfs, residuals, models, gain, threshold, niter, border=0, patch=0, trace=None):
    """psfs [2T - 1, N, N]; residuals and models [T, N, N] float64, updated in place.  Returns the 8 stats [iterations,
    a_0 at the final peak, its flat index, flux_0 .. flux_3, reason].  trace, a list, receives per component (k, the
    relative gap between the two largest scores)."""
    T, N = residuals.shape[0], residuals.shape[1]
    assert psfs.shape == (2 * T - 1, N, N) and models.shape == residuals.shape
    c = N // 2
    Hinv, ok = invert([[psfs[t + q][c, c] for q in range(T)] for t in range(T)])
    if not ok:
        return np.array([0.0, np.nan, -1.0, 0.0, 0.0, 0.0, 0.0, 3.0])
    iters, flux = 0, [0.0, 0.0, 0.0, 0.0]
    while True:
        with np.errstate(invalid="ignore", over="ignore"):
            a = coefficients(Hinv, residuals)
            s = score(a, residuals)
        k, second = clean_ref.peak(s, border)  # (the largest |s|, ties to the lowest flat index, NaN never)
        if k < 0:
            return np.array([iters, np.nan, -1.0] + flux + [2.0])
        y, x = divmod(k, N)
        p = a[0][y, x]
        if not abs(p) > threshold:
            return np.array([iters, p, float(k)] + flux + [1.0])
        if iters >= niter:
            return np.array([iters, p, float(k)] + flux + [0.0])
        if trace is not None:
            top = abs(s[y, x])
            trace.append((k, (top - second) / top if top > 0 else 0.0))
        f = [gain * a[t][y, x] for t in range(T)]
        for t in range(T):
            models[t][y, x] += f[t]
            flux[t] += f[t]
        ylo, yhi = max(0, y - c), min(N - 1, y - c + N - 1)
        xlo, xhi = max(0, x - c), min(N - 1, x - c + N - 1)
        if patch > 0:
            ylo, yhi, xlo, xhi = max(ylo, y - patch), min(yhi, y + patch), max(xlo, x - patch), min(xhi, x + patch)
        for t in range(T):
            for q in range(T):  # (each product is rounded, then subtracted: numpy does not fuse the two)
                residuals[t][ylo:yhi + 1, xlo:xhi + 1] -= f[q] * psfs[t + q][ylo - y + c:yhi - y + c + 1,
                                                                              xlo - x + c:xhi - x + c + 1]
        iters += 1


def midway_threshold(psfs, img, border=0, patch=0):
    """A threshold that a clean of img reaches after some components and before many: half of |a_0| at the first peak,
    which is what a run with niter = 0 reports.  (Half of the image's peak serves for up to three terms; with four the
    coefficient a_0 at the first peak is already below it.)"""
    return 0.5 * abs(mfclean(psfs, img.copy(), np.zeros_like(img), 1.0, 0.0, 0, border, patch)[1])


def make_psfs(N, seed, T, fill=0.04):
    """The 2T - 1 spectral PSFs of clean_ref.make_psf's coverage: every occupied uv cell gets a random x in [-0.25, 0.25],
    term s has the point-symmetrised weights occ * x^s, and all terms are divided by P_0[c, c].  make_psfs(N, seed, 1)[0]
    is clean_ref.make_psf(N, seed)."""
    rng = np.random.default_rng(seed)
    c = N // 2
    yy, xx = np.mgrid[0:N, 0:N]
    r2 = ((yy - c) ** 2 + (xx - c) ** 2) / float(c * c)
    occ = (rng.random((N, N)) < fill * np.exp(-2.0 * r2)).astype(np.float64)
    x = rng.uniform(-0.25, 0.25, (N, N))
    idx = (2 * c - np.arange(N)) % N
    out = []
    for s in range(2 * T - 1):
        w = occ * x ** s
        w = w + w[idx][:, idx]
        out.append(np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(w))).real)
    out = np.ascontiguousarray(np.stack(out) / out[0][c, c])
    assert np.argmax(out[0]) == c * N + c and out[0][c, c] == 1.0
    return out


def make_sky(psfs, seed, nsrc=12, noise=1e-3):
    """(dirty images [T, N, N], source list): nsrc point sources in the inner half with amplitude a and slope a * alpha,
    alpha in [-1.5, 0.5], laid into term t through P_t and P_{t+1} (the clipped shift mfclean itself subtracts), plus
    Gaussian noise in every term"""
    T = (psfs.shape[0] + 1) // 2
    N = psfs.shape[1]
    c = N // 2
    rng = np.random.default_rng(seed)
    ys, xs = rng.integers(N // 4, N - N // 4, nsrc), rng.integers(N // 4, N - N // 4, nsrc)
    amp = rng.uniform(0.2, 1.0, nsrc) * rng.choice([-1.0, 1.0], nsrc)
    alpha = rng.uniform(-1.5, 0.5, nsrc)
    img = np.zeros((T, N, N))
    for y, x, a, al in zip(ys, xs, amp, alpha):
        ylo, yhi, xlo, xhi = max(0, y - c), min(N - 1, y - c + N - 1), max(0, x - c), min(N - 1, x - c + N - 1)
        cut = (slice(ylo - y + c, yhi - y + c + 1), slice(xlo - x + c, xhi - x + c + 1))
        for t in range(T):
            img[t, ylo:yhi + 1, xlo:xhi + 1] += a * psfs[t][cut]
            if t + 1 < 2 * T - 1:
                img[t, ylo:yhi + 1, xlo:xhi + 1] += a * al * psfs[t + 1][cut]
    img += noise * rng.normal(size=(T, N, N))
    return img, list(zip(ys, xs, amp, alpha))
