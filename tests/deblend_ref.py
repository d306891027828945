"""Deblending restated in numpy, rule by rule as include/gridhip.h ("source finding", DEBLENDING) defines it: the up-pointer
of every cell of K, the summits' windows, the ascent to a peak, and one row per peak measured by sources_ref's own measure
and derive over the basin's cells.  The reference the deblending tests compare the library with."""
import numpy as np

import sources_ref

BLENDED = 8  # flag bit 3: the row's island has more than one row


def basins(image, ll, K, T_hi, r):
    """-> sub, N x N int64: on K the flat index of the peak whose basin the cell lies in, -1 elsewhere"""
    N = image.shape[0]
    v, lab, inK = image.ravel(), ll.ravel(), K.ravel()
    cells = [int(k) for k in np.flatnonzero(inK)]

    def higher(a, b):  # image_stats' key order: the value, the smaller index among equals
        return v[a] > v[b] or (v[a] == v[b] and a < b)

    def best_of(k, reach):
        y, x = divmod(k, N)
        best = k
        for ey in range(max(y - reach, 0), min(y + reach, N - 1) + 1):
            for ex in range(max(x - reach, 0), min(x + reach, N - 1) + 1):
                e = ey * N + ex
                if inK[e] and lab[e] == lab[k] and higher(e, best):
                    best = e
        return best

    up = {k: best_of(k, 1) for k in cells}
    brightest = {}
    for k in cells:
        L = int(lab[k])
        if L not in brightest or higher(k, brightest[L]):
            brightest[L] = k
    for k in [k for k in cells if up[k] == k]:  # (decided from the image alone: the order of the summits is immaterial)
        W = best_of(k, r)
        if W != k:
            up[k] = W
        elif not v[k] > T_hi:
            up[k] = brightest[int(lab[k])]
    sub = np.full(N * N, -1, dtype=np.int64)
    for k in cells:
        p = k
        while up[p] != p:
            assert higher(up[p], p)
            p = up[p]
        sub[k] = p
    return sub.reshape(N, N)


def find_sources(image, theta, deblend, sigma=None, border=0, thr=(0.0, 0.0), nsigma=(5.0, 2.5), peak_frac=0.0, min_cells=1,
                 beam=None, correct=True, max_c=None):
    """sources_ref.find_sources with the option "sources_deblend" = deblend: the same dict, one row per peak"""
    if deblend == 0:
        return sources_ref.find_sources(image, theta, sigma, border, thr, nsigma, peak_frac, min_cells, beam, correct, max_c)
    image = np.asarray(image, dtype=np.float64)
    N = image.shape[0]
    T_hi, T_lo, P, reason, ll, K = sources_ref.islands(image, sigma, border, thr, nsigma, peak_frac, min_cells)
    if reason != 0:
        return dict(comps=np.zeros((0, sources_ref.COMP)), info=np.zeros((0, sources_ref.INFO)), count=0,
                    mags=np.zeros((0, 6)), cov=np.zeros((0, 3)), stats=np.array([T_hi, T_lo, P, 0.0, 0.0, 0.0, 0.0, float(reason)]))
    sub = basins(image, ll, K, T_hi, deblend).ravel()
    peaks = np.unique(sub[sub >= 0])  # ascending
    per_island = {}
    for p in peaks:
        per_island[int(ll.ravel()[p])] = per_island.get(int(ll.ravel()[p]), 0) + 1
    rows = peaks.size if max_c is None else min(peaks.size, int(max_c))
    comps, info, mags, covs = [], [], [], []
    for p in peaks[:rows]:
        row, mag = sources_ref.measure(image, np.flatnonzero(sub == p), N)
        assert (row[2], row[3]) == divmod(int(p), N)
        row[0] = float(ll.ravel()[p])  # the island's label, not the basin's first cell
        comp, flags, cov = sources_ref.derive(row, T_lo, theta, N, border, beam, correct)
        if per_island[int(row[0])] > 1:
            flags |= BLENDED
        comps.append(comp)
        info.append(row + [float(flags)])
        mags.append(mag)
        covs.append(cov)
    comps = np.array(comps, dtype=np.float64).reshape(rows, sources_ref.COMP)
    flux = 0.0
    for f in comps[:, 2]:
        flux += float(f)
    points = float(np.count_nonzero((comps[:, 6] == 0.0) & (comps[:, 7] == 0.0)))
    stats = np.array([T_hi, T_lo, P, float(peaks.size), float(rows), points, flux, 0.0])
    return dict(comps=comps, info=np.array(info, dtype=np.float64).reshape(rows, sources_ref.INFO), count=int(peaks.size),
                stats=stats, mags=np.array(mags, dtype=np.float64).reshape(rows, 6),
                cov=np.array(covs, dtype=np.float64).reshape(rows, 3))
