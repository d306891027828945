"""Robust image statistics restated in numpy, statement by statement as include/gridhip.h ("image statistics") defines
them: the reference the image_stats tests compare the library with, bit for bit.  The cells are ordered by the integer key
of their bits, never by comparing doubles, so that -0.0 comes before +0.0 as the header says."""
import numpy as np

TOP = np.uint64(1) << np.uint64(63)


def keys(x):
    """the order-preserving 64-bit key of each double: all bits of a negative value flipped, the sign bit of a
    non-negative value flipped"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((b & TOP) != 0, ~b, b | TOP)


def values(k):
    """the doubles of these keys"""
    k = np.asarray(k, dtype=np.uint64)
    return np.where((k & TOP) != 0, k & ~TOP, ~k).astype(np.uint64).view(np.float64)


def lower_median(x):
    """the element of rank (n - 1) // 2 of the 1-d float64 array x under the key order"""
    k = np.sort(keys(x))
    return float(values(k[(k.size - 1) // 2:(k.size - 1) // 2 + 1])[0])


def image_stats(image, mask=None, border=0):
    """the 8 stats: [n, median, MAD, sigma, min, max, non-finite cells skipped, 0]"""
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    take = np.zeros((N, N), dtype=bool)
    take[border:N - border, border:N - border] = True
    if mask is not None:
        take &= np.asarray(mask) != 0
    skipped = int(np.count_nonzero(take & ~np.isfinite(image)))
    x = image[take & np.isfinite(image)]
    n = x.size
    if n == 0:
        return np.array([0.0, np.nan, np.nan, np.nan, np.nan, np.nan, float(skipped), 0.0])
    k = np.sort(keys(x))
    median = float(values(k[(n - 1) // 2:(n - 1) // 2 + 1])[0])
    with np.errstate(over="ignore"):
        d = np.abs(x - median)  # (the difference rounded once; it may overflow to +Inf, which still has its key)
    mad = lower_median(d)
    lo, hi = (float(v) for v in values(k[[0, -1]]))
    return np.array([float(n), median, mad, 1.4826 * mad, lo, hi, float(skipped), 0.0])
