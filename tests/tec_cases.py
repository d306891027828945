"""Deterministic inputs shared by tests/test_tec_host.py and tests/test_gpu_tec.py: a unit point source at the phase centre
seen through per-antenna clock delays, TEC and phases.  Antenna 0 is the reference."""
import numpy as np

import tec_ref as tr


def pairs(A):
    p, q = np.triu_indices(A, 1)
    return p.astype(np.int64), q.astype(np.int64)


def band(F=32, lo=120.0e6, hi=180.0e6, jitter=0.0, seed=3):
    """F channels from lo to hi (Hz); jitter: the fraction of a step by which every channel but the ends is moved"""
    freq = np.linspace(lo, hi, F) if F > 1 else np.array([0.5 * (lo + hi)])
    if jitter and F > 2:
        freq[1:-1] += jitter * (hi - lo) / (F - 1) * np.random.default_rng(seed).uniform(-1, 1, F - 2)
    return freq


def truth(A, I, freq, seed=11, frac=0.1, tec_max=0.2):
    """(clock [I][A], tec [I][A], phase [I][A]): clock delays within `frac` of the unambiguous range 1 / step, TEC within
    tec_max TEC units, antenna 0 all zero"""
    rng = np.random.default_rng(seed)
    df = np.median(np.diff(freq)) if len(freq) > 1 else 1.0e6
    clock = rng.uniform(-frac, frac, (I, A)) / df
    tec = rng.uniform(-tec_max, tec_max, (I, A))
    ph = rng.uniform(-np.pi, np.pi, (I, A))
    clock[:, 0], tec[:, 0], ph[:, 0] = 0.0, 0.0, 0.0
    return clock, tec, ph


def as_sol(true, freq, orthogonal=True):
    """the truth as a solution [I][A][4] = { tau_eff = clock + s tec, tec, Re g, Im g } of the table's model"""
    clock, tec, ph = true
    _, _, _, s = tr.coordinates(freq, orthogonal)
    return np.stack([clock + s * tec, tec, np.cos(ph), np.sin(ph)], axis=-1)


def corrupt(true, a1, a2, freq, T, tint, amp=1.0):
    """the cube [B][T][F] of a unit point source seen through the physical model: a clock delay and the raw dispersive
    phase -2 pi kappa tec (1 / nu - 1 / nu0)"""
    clock, tec, ph = true
    tint, I = tr.intervals(T, tint)
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    a, z = freq - nu0, -tr.KAPPA * (1.0 / freq - 1.0 / nu0)
    vis = np.zeros((len(a1), T, len(freq)), dtype=np.complex128)
    for i in range(I):
        ta, tb = i * tint, min(T, (i + 1) * tint)
        psi = ph[i][:, None] + 2 * np.pi * clock[i][:, None] * a[None, :] + 2 * np.pi * tec[i][:, None] * z[None, :]
        vis[:, ta:tb] = amp * np.exp(1j * (psi[a1] - psi[a2]))[:, None, :]
    return vis


def errors(sol, want, delays, tecs):
    """the largest delay and TEC errors in cells and the largest phasor error"""
    dg = np.sqrt((sol[..., 2] - want[..., 2]) ** 2 + (sol[..., 3] - want[..., 3]) ** 2)
    return (np.abs(sol[..., 0] - want[..., 0]).max() / delays[1], np.abs(sol[..., 1] - want[..., 1]).max() / tecs[1],
            dg.max())


def recovery_case(flag_fraction=0.0, seed=5, orthogonal=True):
    """the host test's setup: 6 antennas, T = 4, F = 32 over 120-180 MHz, pad = 4, tec_max = 0.5"""
    A, T, F = 6, 4, 32
    a1, a2 = pairs(A)
    freq = band(F)
    delays, tecs = tr.tec_grid(freq, 0.5, pad=4)
    true = truth(A, 1, freq)
    vis = corrupt(true, a1, a2, freq, T, 0)
    wt = None
    if flag_fraction:
        wt = (np.random.default_rng(seed).uniform(size=vis.shape) >= flag_fraction).astype(np.float64)
    tb = tr.tables(freq, T, 0, *delays, *tecs, orthogonal=orthogonal)
    return dict(A=A, T=T, a1=a1, a2=a2, freq=freq, delays=delays, tecs=tecs, true=true, sol=as_sol(true, freq, orthogonal),
                vis=vis, wt=wt, tables=tb)


def composition_case():
    """recovery_case with antenna clocks and TEC a fixed step apart, so that every baseline's band average is wiped out
    before the correction"""
    c = recovery_case(0.0)
    clock, tec, ph = (x.copy() for x in c["true"])
    df = np.median(np.diff(c["freq"]))
    clock[0] = 0.09 * np.arange(c["A"]) / df
    tec[0] = 0.07 * np.arange(c["A"])[::-1]
    tec[0] -= tec[0, 0]
    c["true"] = (clock, tec, ph)
    c["sol"], c["vis"] = as_sol(c["true"], c["freq"]), corrupt(c["true"], c["a1"], c["a2"], c["freq"], c["T"], 0)
    return c
