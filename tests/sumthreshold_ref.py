"""A numpy restatement of time-frequency flagging (include/gridhip.h, "time-frequency flagging"): what the GPU tests compare
with, bit for bit.  Every step is the header's: the classes in their order, the amplitude and the lower medians of
flag_ref.py (a sort), e = a - med, chi_k = levels[k] * (1.4826 * MAD), the window sums as the doubling tree
S = S[..., :-m] + S[..., m:], a window hit when C > 0 and S > chi * C, and the SIR operator in int64."""
import numpy as np

from flag_ref import amplitude, lower_median, same_bits  # noqa: F401

KEPT, FLAGGED, NOT_FINITE, SIR, SUMTHRESHOLD = 0, 1, 3, 8, 16


def ladder(nsigma=6.0, rho=1.5, nlevels=7):
    """the paper's thresholds: chi_k / sigma = nsigma / rho^k for the window 2^k"""
    return np.array([float(nsigma) / float(rho) ** k for k in range(int(nlevels))], dtype=np.float64)


def window_hits(x, c, chi, M):
    """x, c: [..., L] along the last axis; chi broadcasts against [..., 1].  -> the samples hit by a window of length M"""
    L = x.shape[-1]
    hit = np.zeros(x.shape, dtype=bool)
    if M > L:
        return hit
    S, C = x, c
    m = 1
    while m < M:
        S = S[..., :-m] + S[..., m:]
        C = C[..., :-m] + C[..., m:]
        m *= 2
    with np.errstate(invalid="ignore"):
        win = (C > 0) & (S > chi * C.astype(np.float64))  # the starts 0 .. L - M
    for d in range(M):
        hit[..., d:d + L - M + 1] |= win
    return hit


def sir_rows(codes, eta):
    """the SIR operator along the last axis of `codes` (a view is written in place)"""
    if eta == 0.0:
        return
    q = np.int64(np.rint(eta * 2.0 ** 20))
    w = np.where(codes == FLAGGED, np.int64(0), np.where(codes == KEPT, q - np.int64(1 << 20), q)).astype(np.int64)
    P = np.concatenate([np.zeros(codes.shape[:-1] + (1,), dtype=np.int64), np.cumsum(w, axis=-1)], axis=-1)
    lo = np.minimum.accumulate(P[..., :-1], axis=-1)                      # min over i <= x
    hi = np.maximum.accumulate(P[..., :0:-1], axis=-1)[..., ::-1]          # max over j > x
    codes[(codes == KEPT) & (hi - lo >= 0)] = SIR


def sumthreshold(vis, model_vis=None, weights=None, levels=None, nsigma=6.0, rho=1.5, nlevels=7, eta=(0.2, 0.2),
                 min_count=8, niter=2, before_sir=None):
    """vis [B][T][F] -> (wt_out, flags, baseline_stats, stats) as gridhip_sumthreshold leaves them for order 0.
    before_sir: a list that receives a copy of the codes as the rounds left them."""
    vis = np.asarray(vis, dtype=np.complex128)
    B, T, F = vis.shape
    levels = ladder(nsigma, rho, nlevels) if levels is None else np.asarray(levels, dtype=np.float64)
    a = amplitude(vis, model_vis).reshape(B, T, F)
    s = np.ones((B, T, F)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(B, T, F)
    codes = np.zeros((B, T, F), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        codes[~(s > 0.0)] = FLAGGED
    codes[(codes == KEPT) & ~np.isfinite(a)] = NOT_FINITE
    start = int((codes == KEPT).sum())
    bstats = np.empty((B, 4))
    bstats[:] = (0.0, np.nan, np.nan, np.inf)
    if niter == 0:
        bstats[:, 0] = (codes == KEPT).reshape(B, -1).sum(1)
    rounds = flagged = 0
    for r in range(niter):
        rounds += 1
        med, sigma, on = np.zeros(B), np.zeros(B), np.zeros(B, dtype=bool)
        for b in range(B):
            ab = a[b][codes[b] == KEPT]
            if len(ab) == 0:
                bstats[b] = (0.0, np.nan, np.nan, np.inf)
                continue
            med[b] = lower_median(ab)
            mad = lower_median(np.abs(ab - med[b]))
            sigma[b] = np.float64(1.4826) * mad
            on[b] = not (len(ab) < min_count or sigma[b] == 0.0)
            bstats[b] = (len(ab), med[b], mad, levels[0] * sigma[b] if on[b] else np.inf)
        with np.errstate(all="ignore"):
            e = a - med[:, None, None]
        new_in_round = 0
        for k, level in enumerate(levels):
            part = codes == KEPT
            x = np.where(part, e, 0.0)
            c = part.astype(np.int64)
            chi = (level * sigma)[:, None, None]
            hit = window_hits(x, c, chi, 1 << k)                                                     # along frequency
            hit |= window_hits(x.transpose(0, 2, 1), c.transpose(0, 2, 1), chi, 1 << k).transpose(0, 2, 1)  # along time
            new = hit & part & on[:, None, None]
            codes[new] = SUMTHRESHOLD + 8 * r + k
            new_in_round += int(new.sum())
        flagged += new_in_round
        if new_in_round == 0:
            break
    if before_sir is not None:
        before_sir.append(codes.copy())
    not_sir = codes != KEPT
    sir_rows(codes, float(eta[0]))
    sir_rows(codes.transpose(0, 2, 1), float(eta[1]))
    added = int((codes != KEPT).sum() - not_sir.sum())
    wt_out = np.where(codes == KEPT, s, 0.0)
    stats = np.array([rounds, start, flagged, (codes == NOT_FINITE).sum(), added, 0, (codes == FLAGGED).sum(),
                      start - flagged - added], dtype=np.float64)
    return wt_out, codes, bstats, stats


def interference_cube(seed, shape=(4, 96, 160)):
    """the cube of the quality check: unit complex Gaussian noise with a burst, a line and a spike added to the amplitudes,
    and a channel flagged on input -> (vis, weights, injected)"""
    rng = np.random.default_rng(seed)
    vis = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    add = np.zeros(shape)
    add[1, 10:14, :] += 1.5
    add[2, :, 50] += 1.0
    add[3, 40, 70] += 12.0
    amp = np.abs(vis)
    vis = vis * ((amp + add) / amp)
    wt = np.ones(shape)
    wt[0, :, 100] = 0.0
    return vis, wt, add > 0
