"""Deterministic inputs shared by tests/test_fringe_host.py and tests/test_gpu_fringe.py: a point source at the phase
centre seen through per-antenna delays, rates and phases."""
import numpy as np

import fringe_ref as fr


def pairs(A):
    p, q = np.triu_indices(A, 1)
    return p.astype(np.int64), q.astype(np.int64)


def axes(T=8, F=16, jitter=0.0, seed=3):
    """freq (Hz) and time (s); jitter: the fraction of a step by which every value but the ends is moved"""
    rng = np.random.default_rng(seed)
    freq, time = 1.0e9 + 1.0e6 * np.arange(F), 2.0 * np.arange(T)
    if jitter:
        freq[1:-1] += jitter * 1.0e6 * rng.uniform(-1, 1, max(F - 2, 0))
        time[1:-1] += jitter * 2.0 * rng.uniform(-1, 1, max(T - 2, 0))
    return freq, time


def truth(A, I, freq, time, seed=11, frac=0.1):
    """[I][A][4] = tau, r, Re g, Im g: delays and rates within `frac` of the unambiguous ranges 1 / step, antenna 0 the
    reference (all zero), so that
    every true value lies within 0.1 of the range"""
    rng = np.random.default_rng(seed)
    df, dt = np.median(np.diff(freq)), (np.median(np.diff(time)) if len(time) > 1 else 1.0)
    sol = np.zeros((I, A, 4))
    sol[:, :, 0] = rng.uniform(-frac, frac, (I, A)) / df
    sol[:, :, 1] = rng.uniform(-frac, frac, (I, A)) / dt
    ph = rng.uniform(-np.pi, np.pi, (I, A))
    sol[:, 0, :2], ph[:, 0] = 0.0, 0.0
    sol[:, :, 2], sol[:, :, 3] = np.cos(ph), np.sin(ph)
    return sol


def corrupt(sol, a1, a2, freq, time, tint, amp=1.0):
    """the cube [B][T][F] of a unit point source seen through `sol`"""
    T, F = len(time), len(freq)
    tint, I = fr.intervals(T, tint)
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    vis = np.zeros((len(a1), T, F), dtype=np.complex128)
    for i in range(I):
        ta, tb = i * tint, min(T, (i + 1) * tint)
        tref = time[ta] + 0.5 * (time[tb - 1] - time[ta])
        psi = (np.arctan2(sol[i, :, 3], sol[i, :, 2])[:, None, None]
               + 2 * np.pi * sol[i, :, 0][:, None, None] * (freq - nu0)[None, None, :]
               + 2 * np.pi * sol[i, :, 1][:, None, None] * (time[ta:tb] - tref)[None, :, None])
        vis[:, ta:tb] = amp * np.exp(1j * (psi[a1] - psi[a2]))
    return vis


def errors(sol, true, delays, rates):
    """the largest delay and rate errors in cells and the largest phasor error"""
    dg = np.sqrt((sol[..., 2] - true[..., 2]) ** 2 + (sol[..., 3] - true[..., 3]) ** 2)
    return (np.abs(sol[..., 0] - true[..., 0]).max() / delays[1], np.abs(sol[..., 1] - true[..., 1]).max() / rates[1],
            dg.max())


def recovery_case(flag_fraction=0.0, seed=5):
    """the host test's setup: 6 antennas, T = 8, F = 16, pad = 4 -> everything a fit needs"""
    A, T, F = 6, 8, 16
    a1, a2 = pairs(A)
    freq, time = axes(T, F)
    delays, rates = fr.fringe_grid(freq, time, 0, pad=4)
    true = truth(A, 1, freq, time)
    vis = corrupt(true, a1, a2, freq, time, 0)
    wt = None
    if flag_fraction:
        wt = (np.random.default_rng(seed).uniform(size=vis.shape) >= flag_fraction).astype(np.float64)
    tb = fr.tables(freq, time, 0, *delays, *rates)
    return dict(A=A, a1=a1, a2=a2, freq=freq, time=time, delays=delays, rates=rates, true=true, vis=vis, wt=wt, tables=tb)


def composition_case():
    """recovery_case with antenna delays and rates a fixed step apart, so that every baseline's band-and-time average is
    wiped out before the correction"""
    c = recovery_case(0.0)
    true = c["true"].copy()
    true[0, :, 0] = 0.09 * np.arange(c["A"]) / 1.0e6
    true[0, :, 1] = 0.07 * np.arange(c["A"])[::-1] / 2.0
    true[0, :, 1] -= true[0, 0, 1]
    c["true"], c["vis"] = true, corrupt(true, c["a1"], c["a2"], c["freq"], c["time"], 0)
    return c
