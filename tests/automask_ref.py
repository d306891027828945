"""Auto-masking restated in numpy and a plain flood fill, step by step as include/gridhip.h ("auto-masking") defines it:
the reference the automask tests compare the library with - the mask byte for byte, the stats bit for bit."""
import numpy as np

import noise_ref

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def label(inset):
    """The 8-connected components of the boolean N x N array `inset` by a flood fill from every cell in row-major
    order: an int64 array holding, for a cell of the set, the smallest flat index k = y * N + x of its component, and -1
    outside the set."""
    inset = np.asarray(inset, dtype=bool)
    H, W = inset.shape
    out = np.full((H, W), -1, dtype=np.int64)
    for y0 in range(H):
        for x0 in range(W):
            if not inset[y0, x0] or out[y0, x0] >= 0:
                continue
            root = y0 * W + x0  # the first cell met in row-major order is the component's smallest index
            out[y0, x0] = root
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in NEIGHBOURS:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and inset[yy, xx] and out[yy, xx] < 0:
                        out[yy, xx] = root
                        stack.append((yy, xx))
    return out


def grow_set(K, g):
    """the cells within Chebyshev distance g of a cell of K"""
    H, W = K.shape
    G = np.zeros_like(K)
    for dy in range(-g, g + 1):
        for dx in range(-g, g + 1):
            ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
            xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
            G[yd, xd] |= K[ys, xs]
    return G


def automask(image, mask, sigma=None, border=0, absolute=False, thr=(0.0, 0.0), nsigma=(5.0, 2.5), peak_frac=0.0,
             min_cells=1, grow=0):
    """-> (the updated mask, a new uint8 array; the 8 stats).  sigma None stands for a NULL noise (both nsigma 0)."""
    image = np.asarray(image, dtype=np.float64)
    mask = np.asarray(mask).view(np.uint8) if np.asarray(mask).dtype == bool else np.asarray(mask, dtype=np.uint8)
    out = mask.copy()
    N = image.shape[0]
    region = np.zeros((N, N), dtype=bool)
    region[border:N - border, border:N - border] = True
    part = region & np.isfinite(image)
    v = np.abs(image) if absolute else image
    T_hi, T_lo = float(thr[0]), float(thr[1])
    P = np.nan
    if part.any():
        P = float(noise_ref.values(noise_ref.keys(v[part]).max(keepdims=True))[0])
    if nsigma[0] > 0.0:
        sigma = float(sigma)
        if sigma != sigma:
            return out, np.array([np.nan, np.nan, P, 0.0, 0.0, 0.0, 0.0, 3.0])
        T_hi = max(T_hi, float(np.float64(nsigma[0]) * np.float64(sigma)))
        if nsigma[1] > 0.0:
            T_lo = max(T_lo, float(np.float64(nsigma[1]) * np.float64(sigma)))
    if not part.any():
        return out, np.array([T_hi, T_lo, P, 0.0, 0.0, 0.0, 0.0, 2.0])
    if peak_frac > 0.0:
        c = float(np.float64(peak_frac) * np.float64(P))
        T_hi, T_lo = max(T_hi, c), max(T_lo, c)
    with np.errstate(invalid="ignore"):
        Hs, Ls = part & (v > T_hi), part & (v > T_lo)
    lh = label(Hs)
    roots, sizes = np.unique(lh[lh >= 0], return_counts=True)
    alive = roots[sizes >= min_cells]
    S = np.isin(lh, alive) & Hs
    ll = label(Ls)
    kept = np.unique(ll[S])
    K = np.isin(ll, kept) & Ls
    G = grow_set(K, int(grow)) & region
    new = G & (out == 0)
    out[new] = 1
    return out, np.array([T_hi, T_lo, P, float(roots.size), float(alive.size), float(kept.size),
                          float(np.count_nonzero(new)), 0.0])
