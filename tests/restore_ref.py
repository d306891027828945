"""The restoring beam and the restore restated in numpy, statement by statement as include/gridhip.h ("restoring beam and
restore") defines them: the reference the restore tests compare the library with.  The reference project stops at the
dirty image, so this restatement is the only other implementation; tests/test_restore_host.py checks it on cases
computed by hand."""
import math

import numpy as np

NAN8 = [np.nan] * 6


def normal_equations(psf, window, cut):
    """(M, g, ncells, pc): the 3 x 3 normal matrix, the right-hand side's negative and the number of participating cells of
    the fit, summed as the header orders it - each row dy in dx order from +0.0, then the rows in dy order - and the
    PSF's centre value"""
    N = psf.shape[0]
    c = N // 2
    R = min(window, c, N - 1 - c)
    pc = psf[c, c]
    tot = [0.0] * 10
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            s = [0.0] * 10
            for dx in range(-R, R + 1):
                if dy == 0 and dx == 0:
                    continue
                p = float(psf[c + dy, c + dx] / pc)
                near = max(abs(dy), abs(dx)) == 1
                if not (p <= 1.0 and (p >= cut or (near and p > 0.0))):  # (a NaN fails p <= 1)
                    continue
                w, l = p * p, math.log(p)
                a, b, cc = float(dx * dx), float(2 * dx * dy), float(dy * dy)
                wa, wb, wc = w * a, w * b, w * cc
                for i, v in enumerate((wa * a, wa * b, wa * cc, wb * b, wb * cc, wc * cc, wa * l, wb * l, wc * l, 1.0)):
                    s[i] += v
            for i in range(10):
                tot[i] += s[i]
    M = np.array([[tot[0], tot[1], tot[2]], [tot[1], tot[3], tot[4]], [tot[2], tot[4], tot[5]]])
    return M, np.array(tot[6:9]), tot[9], float(pc)


def derived(A, B, C):
    """(bmaj, bmin, bpa) of the form [[A, B], [B, C]] as the header defines them"""
    h, d = 0.5 * (A + C), 0.5 * (A - C)
    q = math.sqrt(d * d + B * B)
    pa = 0.0 if (A == C and B == 0.0) else 0.5 * math.atan2(0.0 - 2.0 * B, C - A)
    if pa <= -0.5 * math.pi:
        pa += math.pi
    return 2.0 * math.sqrt(math.log(2.0) / (h - q)), 2.0 * math.sqrt(math.log(2.0) / (h + q)), pa


def fit_beam(psf, window, cut):
    """-> the 8 doubles [A, B, C, bmaj, bmin, bpa, ncells, ok]"""
    M, g, ncells, pc = normal_equations(psf, window, cut)
    (m00, m01, m02), (_, m11, m12), (_, _, m22) = M.tolist()
    r0, r1, r2 = (-g).tolist()
    with np.errstate(all="ignore"):
        c00, c01, c02 = m11 * m22 - m12 * m12, m01 * m22 - m12 * m02, m01 * m12 - m11 * m02
        det = np.float64(m00 * c00 - m01 * c01 + m02 * c02)
        A = float((r0 * c00 - m01 * (r1 * m22 - m12 * r2) + m02 * (r1 * m12 - m11 * r2)) / det)
        B = float((m00 * (r1 * m22 - m12 * r2) - r0 * c01 + m02 * (m01 * r2 - r1 * m02)) / det)
        C = float((m00 * (m11 * r2 - r1 * m12) - m01 * (m01 * r2 - r1 * m02) + r0 * c02) / det)
    ok = (ncells >= 3 and det > 0.0 and 0.0 < pc < math.inf and 0.0 < A < math.inf and 0.0 < C < math.inf
          and A * C - B * B > 0.0)
    if not ok:
        return np.array(NAN8 + [ncells, 0.0])
    return np.array([A, B, C, *derived(A, B, C), ncells, 1.0])


def beam_usable(beam):
    A, B, C, ok = (float(beam[i]) for i in (0, 1, 2, 7))
    return bool(ok != 0.0 and ok == ok and 0.0 < A < math.inf and 0.0 < C < math.inf and math.isfinite(B)
                and A * C - B * B > 0.0)


def weights(beam, support):
    """beam(dy, dx) over |dy|, |dx| <= support, [dy + support][dx + support]"""
    A, B, C = (float(beam[i]) for i in range(3))
    d = np.arange(-support, support + 1, dtype=np.float64)
    dy, dx = d[:, None], d[None, :]
    return np.exp(-(A * dx * dx + 2.0 * B * dx * dy + C * dy * dy))


def restore(model, residual, beam, support):
    """-> (restored, magnitude): restored = residual + sum of model[y - dy, x - dx] * beam(dy, dx), the taps dy ascending,
    then dx ascending from +0.0, the residual added last; magnitude = |residual| + sum of |model| * beam, per cell (what
    the rounding errors of the sum scale with).  An unusable beam gives NaN everywhere."""
    N = model.shape[0]
    if not beam_usable(beam):
        return np.full((N, N), np.nan), np.full((N, N), np.nan)
    w = weights(beam, support)
    s = support
    pad = np.zeros((N + 2 * s, N + 2 * s))
    pad[s:s + N, s:s + N] = model
    apad = np.abs(pad)
    acc, mag = np.zeros((N, N)), np.zeros((N, N))
    with np.errstate(invalid="ignore"):
        for dy in range(-s, s + 1):
            for dx in range(-s, s + 1):
                acc += pad[s - dy:s - dy + N, s - dx:s - dx + N] * w[dy + s, dx + s]
                mag += apad[s - dy:s - dy + N, s - dx:s - dx + N] * w[dy + s, dx + s]
        return residual + acc, np.abs(residual) + mag


def smooth_psf(N, seed, s, q=1.0, ang=0.0):
    """A PSF with a resolved main lobe: a Gaussian uv taper of width s (in units of the half grid; q: the axis ratio, ang:
    its rotation), randomly perturbed and made point-symmetric about the centre cell so that the PSF is real, through
    the centred inverse transform, normalised to 1 at the zero-lag cell (N // 2, N // 2)."""
    rng = np.random.default_rng(seed)
    c = N // 2
    yy, xx = np.mgrid[0:N, 0:N]
    v, u = (yy - c) / float(c), (xx - c) / float(c)
    ur, vr = u * math.cos(ang) + v * math.sin(ang), -u * math.sin(ang) + v * math.cos(ang)
    w = np.exp(-0.5 * ((ur / s) ** 2 + (vr / (s * q)) ** 2)) * (1.0 + 0.2 * rng.random((N, N)))
    idx = (2 * c - np.arange(N)) % N
    w = w + w[idx][:, idx]
    psf = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(w))).real
    psf = psf / psf[c, c]
    assert np.argmax(psf) == c * N + c
    return np.ascontiguousarray(psf)
