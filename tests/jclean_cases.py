"""Inputs that test_jclean_host.py (host) and test_gpu_jclean.py (GPU) share: the exact fixtures at which the joint CLEAN
(jclean.hip) meets tiny images, the rim, odd N - where the planes' slots are 8 bytes apart in alignment - ties between
cells whose planes differ, NaN in one plane, masks, zero weights and stop levels.  No GPU: plain numpy, the restatement
jclean_ref and clean_edge_cases' exact PSF.

Exact fixtures, by clean_edge_cases' rule: the PSFs' cells are signed powers of two (1.0 at the centre), the residuals'
cells small integers, the weights small integers, gain 0.5 or 0.25 and the threshold 0 or a small integer: every product,
square, sum and difference of a run is then exact in fp64, and a correct kernel gives the restatement's BITS whatever it
fuses.  That every operation was exact is not argued but checked, by the host test: the same run in np.longdouble gives
the same numbers."""
import functools
from collections import namedtuple

import numpy as np

import jclean_ref
from clean_edge_cases import exact_psf, rim_cells

# name; N; P, Q; metric (0 sum, 1 sumsq); weights (None: all 1); cells: (p, y, x, value) laid over the fill; fill: "noise"
# (-1 or 1 by a seeded draw per plane), "nan" or a number; mask: cells (y, x) whose byte is 0, "zero" (every byte 0) or None;
# nsigma, sigma, threshold: the stop level's terms
Jx = namedtuple("Jx", "name N P Q metric weights cells fill gain niter border patch mask nsigma sigma threshold")


def jx(name, N, P, Q, metric, cells, weights=None, fill="noise", gain=0.5, niter=5, border=0, patch=0, mask=None,
       nsigma=0.0, sigma=None, threshold=0.0):
    return Jx(name, N, P, Q, metric, None if weights is None else tuple(weights), tuple(cells), fill, gain, niter, border,
              patch, mask if mask is None or mask == "zero" else tuple(mask), nsigma, sigma, threshold)


@functools.lru_cache(maxsize=8)
def exact_psfs(N, Q):
    """Q exact PSFs, 1.0 at the centre: clean_edge_cases.exact_psf, its transpose, the two negated off the centre, and
    the four halved off the centre - a read of another plane's PSF shows"""
    c = N // 2
    e = np.array(exact_psf(N))
    out = []
    for q in range(Q):
        v = (e.T if q & 1 else e) * (-1.0 if q & 2 else 1.0) * (0.5 if q & 4 else 1.0)
        v = v.copy()
        v[c, c] = 1.0
        out.append(v)
    out = np.ascontiguousarray(np.stack(out))
    out.setflags(write=False)
    return out


def residuals_of(f):
    N, P = f.N, f.P
    if f.fill == "noise":
        res = np.random.default_rng(11 * N + P).integers(0, 2, (P, N, N)).astype(np.float64) * 2.0 - 1.0
    else:
        res = np.full((P, N, N), np.nan if f.fill == "nan" else f.fill, dtype=np.float64)
    for p, y, x, v in f.cells:
        res[p, y, x] = v
    return res


def mask_of(f):
    if f.mask is None:
        return None
    m = np.ones((f.N, f.N), dtype=np.uint8)
    if f.mask == "zero":
        m[:] = 0
    else:
        for y, x in f.mask:
            m[y, x] = 0
    return m


def keywords(f):
    """the fixture as Context.jclean's keywords (psfs and images apart)"""
    return dict(metric=("sum", "sumsq")[f.metric], weights=[1.0] * f.P if f.weights is None else list(f.weights),
                gain=f.gain, threshold=f.threshold, niter=f.niter, border=f.border, patch=f.patch, mask=mask_of(f),
                nsigma=f.nsigma, noise=f.sigma)


def reference(f, dtype=np.float64, trace=None):
    """(models, residuals, stats) of fixture f by the restatement, on arrays of `dtype`"""
    psfs, res = exact_psfs(f.N, f.Q).astype(dtype), residuals_of(f).astype(dtype)
    models = np.zeros_like(res)
    kw = {} if dtype is np.float64 else dict(fma=lambda a, b, c: a * b + c)  # (exact either way on these fixtures)
    with np.errstate(invalid="ignore"):
        stats = jclean_ref.jclean(psfs, res, models, f.weights, f.metric, f.gain, f.threshold, f.niter, f.border, f.patch,
                                  mask_of(f), f.nsigma, f.sigma, 0.0, trace, **kw)
    return models, res, stats


def plane_cells(N, P):
    """clean_edge_cases.rim_cells - the four corners and the edge midpoints, so that every update region is clipped - in
    every plane: plane p holds the magnitudes rotated by p places, every other pair of planes negated, so the planes' values
    at a cell differ and the statistic's order of peaks is not any one plane's"""
    base = rim_cells(N)
    out = []
    for p in range(P):
        for i, (y, x, _) in enumerate(base):
            v = base[(i + p) % len(base)][2]
            out.append((p, y, x, abs(v) * (-1.0 if (p // 2 + i) % 2 else 1.0)))
    return out


def size_fixtures():
    """N in 1 .. 5, 17 and 129 (one row or column past a tile; odd N with P >= 2: the planes' slots are 8 bytes apart in
    alignment) and 128; both metrics; one PSF and one per plane; the whole PSF and a patch"""
    out = []
    for N in (1, 2, 3, 4, 5, 17, 128, 129):
        for P, Q, metric in ((2, 2, 0), (3, 1, 1), (3, 3, 1), (8, 8, 0), (4, 1, 1)):
            if P == 8 and N not in (5, 129):
                continue
            for patch in (0, 1):
                out.append(jx(f"size-N{N}-P{P}-Q{Q}-m{metric}-patch{patch}", N, P, Q, metric, plane_cells(N, P), niter=6,
                              patch=patch))
    return out


def tie_fixtures():
    """two cells tied in s with different per-plane values: the lowest flat index wins, whichever plane holds the larger
    value there.  patch = 1 keeps the cells out of each other's update region: they stay tied from pick to pick."""
    out = []
    for N in (129, 300):
        for metric in (0, 1):
            # sum: 5 + 2 = 2 + 5; sumsq: 25 + 4 = 4 + 25
            for name, a, b in (("one-slot", (20, 10 + (20 * N + 10) % 2), None), ("two-rows", (18, 100), (22, 4)),
                               ("two-tiles", (15, 127), (16, 2)), ("later-entry-lower-index", (0, 130 % N), (1, 5))):
                b = (a[0], a[1] + 1) if b is None else b
                cells = [(0, *a, 5.0), (1, *a, 2.0), (0, *b, 2.0), (1, *b, 5.0)]
                out.append(jx(f"tie-{name}-N{N}-m{metric}", N, 2, 2, metric, cells, gain=0.25, niter=4, patch=1))
        # weights 2 and 1, the sum: 2 * 3 + 1 * 4 = 2 * 4 + 1 * 2
        out.append(jx(f"tie-weighted-N{N}", N, 2, 1, 0, [(0, 40, 9, 3.0), (1, 40, 9, 4.0), (0, 30, 90, 4.0), (1, 30, 90, 2.0)],
                      weights=(2.0, 1.0), gain=0.25, niter=4, patch=1))
    return out


def exclusion_fixtures():
    out = []
    for N in (17, 130):
        peak = [(0, 5, 7, 9.0), (1, 5, 7, 9.0), (0, 9, 3, 6.0), (1, 9, 3, -3.0), (2, 9, 3, 6.0)]
        for metric in (0, 1):
            # a NaN in plane 2 only, at the would-be peak: the cell is never selected, and is still updated
            out.append(jx(f"nan-in-plane-2-N{N}-m{metric}", N, 3, 1, metric, peak + [(2, 5, 7, np.nan)], niter=3))
            out.append(jx(f"nan-under-weight-0-N{N}-m{metric}", N, 3, 3, metric, peak + [(2, 5, 7, np.nan)],
                          weights=(1.0, 1.0, 0.0), niter=3))
            out.append(jx(f"all-nan-N{N}-m{metric}", N, 2, 2, metric, [], fill="nan", niter=3))
            out.append(jx(f"one-plane-nan-N{N}-m{metric}", N, 2, 1, metric,
                          [(0, y, x, 1.0) for y in range(N) for x in range(N)], fill="nan", niter=3))
            out.append(jx(f"zero-mask-N{N}-m{metric}", N, 2, 1, metric, peak[:4], mask="zero", niter=3))
            out.append(jx(f"masked-peak-N{N}-m{metric}", N, 3, 1, metric, peak + [(2, 5, 7, 9.0)], mask=[(5, 7), (0, 0)],
                          niter=3, border=1))
            out.append(jx(f"nan-sigma-N{N}-m{metric}", N, 2, 2, metric, peak[:4], nsigma=3.0, sigma=np.nan, niter=3))
            # L = max(2^d, (2 * 5)^d) = 10^d: after one component s = 8 <= 10 (sum), 32 <= 100 (sumsq): reason 1
            out.append(jx(f"stop-level-N{N}-m{metric}", N, 2, 1, metric, [(0, 5, 7, 8.0), (1, 5, 7, 8.0), (0, 9, 3, 4.0)],
                          fill=0.0, nsigma=2.0, sigma=5.0, threshold=2.0, niter=9, patch=2))
    return out


def weight_fixtures():
    """a plane of weight 0 that holds the largest value does not steer the search and is still cleaned; {1, 0, 0, 0}"""
    out = []
    for N in (17, 129):
        cells = [(0, 4, 4, 5.0), (0, 10, 12, -4.0), (1, 8, 8, 40.0), (2, 4, 4, 7.0), (3, 10, 12, -9.0), (3, 2, 15, 30.0)]
        for metric in (0, 1):
            for Q in (1, 4):
                out.append(jx(f"weights-1000-N{N}-Q{Q}-m{metric}", N, 4, Q, metric, cells, weights=(1.0, 0.0, 0.0, 0.0),
                              gain=0.25, niter=5, patch=3))
            out.append(jx(f"weights-0201-N{N}-m{metric}", N, 4, 1, metric, cells, weights=(0.0, 2.0, 0.0, 1.0), gain=0.25,
                          niter=5))
    return out


def all_fixtures():
    return size_fixtures() + tie_fixtures() + exclusion_fixtures() + weight_fixtures()
