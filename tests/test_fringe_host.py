"""The numpy restatement of delay and rate calibration (tests/fringe_ref.py) against independent numpy, and what a fit
recovers from a corrupted point source.  No GPU."""
import numpy as np
import pytest

import fringe_cases as fc
import fringe_ref as fr


@pytest.fixture(scope="module")
def clean():
    return fc.recovery_case(0.0)


@pytest.fixture(scope="module")
def flagged():
    return fc.recovery_case(0.3)


def _complex(x):
    return x[..., 0] + 1j * x[..., 1]


def test_table_is_the_phasors_of_the_definition():
    freq, time = fc.axes(T=7, F=5, jitter=0.3)
    delays, rates = (-3.0e-7, 4.0e-8, 9), (-0.1, 0.03, 6)
    tb = fr.tables(freq, time, 3, *delays, *rates)
    h = fr.split(tb, 7, 5)
    assert (h["tint"], h["I"], h["Nd"], h["Nr"]) == (3, 3, 9, 6)
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    tref = np.array([time[0] + 0.5 * (time[2] - time[0]), time[3] + 0.5 * (time[5] - time[3]), time[6]])
    assert h["nu0"] == nu0 and np.array_equal(h["tref"][:3], tref) and not h["tref"][3:].any()
    tau, r = delays[0] + np.arange(9) * delays[1], rates[0] + np.arange(6) * rates[1]
    want = np.exp(-2j * np.pi * tau[None, :] * (freq - nu0)[:, None])
    assert np.abs(_complex(h["Ef"]) - want).max() < 1e-12  # (the phase is hundreds of turns before the reduction)
    want = np.exp(-2j * np.pi * r[None, :] * (time - tref[np.arange(7) // 3])[:, None])
    assert np.abs(_complex(h["Et"]) - want).max() < 1e-13
    assert len(tb) == fr.table_doubles(5, 7, 9, 6)


def test_invalid_axes_give_an_invalid_table():
    freq, time = fc.axes(T=4, F=4)
    for bad in (dict(dtau=0.0), dict(drate=-1.0), dict(tau0=np.nan), dict(freq=np.array([1.0, np.inf, 3.0, 4.0]))):
        kw = dict(freq=freq, time=time, tau0=0.0, dtau=1e-8, drate=0.1)
        kw.update(bad)
        tb = fr.tables(kw["freq"], time, 0, kw["tau0"], kw["dtau"], 4, 0.0, kw["drate"], 4)
        assert tb[0] == 0.0 and not tb[fr.HEAD:].any() and fr.split(tb, 4, 4) is None


def test_power_at_every_cell_is_einsums(clean):
    c = clean
    h = fr.split(c["tables"], 8, 16)
    rng = np.random.default_rng(2)
    vis = c["vis"] + 0.3 * (rng.normal(size=c["vis"].shape) + 1j * rng.normal(size=c["vis"].shape))
    model = rng.normal(size=vis.shape) + 1j * rng.normal(size=vis.shape)
    wt = rng.uniform(0.5, 2.0, vis.shape) * (rng.uniform(size=vis.shape) > 0.2)
    sol = fc.truth(c["A"], 1, c["freq"], c["time"], seed=4)
    for b in (0, 7, 14):
        p, q = int(c["a1"][b]), int(c["a2"][b])
        x, flagged, t0, nt = fr.samples(h, vis, model, wt, sol, b, 0, p, q)
        s = fr.fringe_power(h, x, t0, nt, 0, h["Nd"], 0, h["Nr"])
        # independent: complex numpy, the derotation as one exponential
        nu0 = c["freq"][0] + 0.5 * (c["freq"][-1] - c["freq"][0])
        tref = c["time"][0] + 0.5 * (c["time"][-1] - c["time"][0])
        g = sol[0, :, 2] + 1j * sol[0, :, 3]
        D = (g[p] * np.conj(g[q]) * np.exp(2j * np.pi * ((sol[0, p, 0] - sol[0, q, 0]) * (c["freq"] - nu0)[None, :]
                                                         + (sol[0, p, 1] - sol[0, q, 1]) * (c["time"] - tref)[:, None])))
        X = np.where(wt[b] > 0, wt[b] * vis[b] * np.conj(model[b]) * np.conj(D), 0.0)
        assert np.array_equal(flagged, ~(wt[b] > 0))
        S = np.einsum("fj,tk,tf->jk", _complex(h["Ef"]), _complex(h["Et"]), X)
        assert np.abs(S - (s[0] + 1j * s[1])).max() <= 1e-12 * np.abs(X).sum()


def test_fringe_grid_values():
    import gridhip
    freq, time = fc.axes(T=8, F=16, jitter=0.2)
    (tau0, dtau, Nd), (r0, drate, Nr) = gridhip.fringe_grid(freq, time, 0, pad=4)
    assert (Nd, Nr) == (64, 32)
    assert dtau == 1.0 / (4 * 16 * np.median(np.abs(np.diff(freq)))) and drate == 1.0 / (4 * 8 * np.median(np.abs(np.diff(time))))
    assert tau0 + 32 * dtau == 0.0 and r0 + 16 * drate == 0.0  # centred: a cell is zero
    assert gridhip.fringe_grid(freq, time, 0, pad=4) == fr.fringe_grid(freq, time, 0, pad=4)
    assert gridhip.fringe_grid(freq, time, 3, pad=2)[1][2] == 6
    with pytest.raises(ValueError):
        gridhip.fringe_grid(np.arange(1, 1025.0), time, 0, pad=8)  # 8192 delays
    with pytest.raises(ValueError):
        gridhip.fringe_grid(freq, time, 300)


def _rounds(c):
    hist = []
    sol, peaks, info, stats = fr.fringefit(c["tables"], c["vis"], c["a1"], c["a2"], c["A"], wt=c["wt"], rounds=3,
                                           window_cells=(2, 2), refant=0, niter=50, history=hist)
    return [fc.errors(s, c["true"], c["delays"], c["rates"]) for _, s in hist], sol, peaks, info, stats


# what the restatement recovers (delay error, rate error in cells; phasor error), measured on these deterministic inputs;
# the asserts stand at twice the measured values, a margin for another seed only:
#   noiseless        round 0: 0.00638, 0.0111      round 2: 4.21e-5, 7.07e-5     phasor 1.2e-16 after every round
#   30 % flagged     round 0: 0.0120, 0.0168       round 2: 6.12e-5, 5.04e-5     phasor 1.0e-2, then 1.16e-5
# (the true delays and rates lie within 0.1 of the unambiguous ranges: fringe_cases.truth)
CLEAN_BOUNDS = ((0.01276, 0.0222), (8.42e-5, 1.414e-4))
FLAGGED_BOUNDS = ((0.0240, 0.0336), (1.224e-4, 1.008e-4))


def test_noiseless_recovery(clean):
    err, sol, peaks, info, stats = _rounds(clean)
    print("noiseless", err)
    assert err[0][0] < CLEAN_BOUNDS[0][0] and err[0][1] < CLEAN_BOUNDS[0][1]
    assert err[2][0] < CLEAN_BOUNDS[1][0] and err[2][1] < CLEAN_BOUNDS[1][1]
    assert max(e[2] for e in err) < 1e-15  # measured 1.2e-16: rounding level
    assert (peaks[:, :, 10] == 0).all() and (info == 5).all() and stats[7] == 0 and stats[4] == 0
    assert (peaks[:, 0, 0] == 32).all() and (peaks[:, 0, 1] == 16).all()  # the last round peaks at the grid's zero
    assert stats[5] < 0.01 and stats[6] < 0.01  # the residuals of the last round, in cells


def test_recovery_with_flags(flagged):
    err, sol, peaks, info, stats = _rounds(flagged)
    print("flagged", err)
    assert err[0][0] < FLAGGED_BOUNDS[0][0] and err[0][1] < FLAGGED_BOUNDS[0][1]
    assert err[2][0] < FLAGGED_BOUNDS[1][0] and err[2][1] < FLAGGED_BOUNDS[1][1]
    assert err[2][2] < 2.32e-5  # measured 1.16e-5
    assert stats[1] == (flagged["wt"] == 0).sum()


def test_search_classes_and_ties(clean):
    c = clean
    vis, wt = c["vis"].copy(), np.ones(c["vis"].shape)
    a1, a2 = c["a1"].copy(), c["a2"].copy()
    vis[1] = 0.0                     # all zero: ok, the tie goes to the first cell, coh2 = 0
    wt[2] = 0.0
    vis[2, 3, 4] = np.nan            # flagged whole, a NaN under a zero weight: empty
    vis[3, 1, 2] = np.nan            # an unflagged NaN: bad
    a2[4] = a1[4]                    # an autocorrelation
    a1[5] = 99                       # out of range
    peaks, stats = fr.search(c["tables"], vis, a1, a2, c["A"], wt=wt, cells=(3, 40, 2, 30))
    assert list(peaks[:6, 0, 10]) == [0, 0, 1, 2, 3, 3]
    assert list(peaks[1, 0, :3]) == [3, 2, 0] and peaks[1, 0, 7] == 0 and list(peaks[1, 0, 5:7]) == [1, 0]
    assert peaks[1, 0, 3] == c["delays"][0] + 3 * c["delays"][1]  # on the edge: the grid value stands
    assert list(stats) == [128, 1, 1, 2, 11, 0, 0, 0]
    w = fr.weights(peaks, a1, a2, c["A"], 0, 0.0, 0.0)
    assert not w[1:6].any() and (w[6:] > 0).all()
    assert fr.search(c["tables"], vis, a1, a2, c["A"], cells=(0, 65, 0, 4))[1][7] == 1  # cells outside the grid


def test_apply_restores_the_source(clean):
    c = clean
    out, wout = fr.apply(c["tables"], c["true"], c["a1"], c["a2"], c["vis"])
    assert np.abs(out - 1.0).max() < 1e-12 and (wout == 1).all()
    back, _ = fr.apply(c["tables"], c["true"], c["a1"], c["a2"], out, inverse=False)
    assert np.abs(back - c["vis"]).max() < 1e-12
    sol = c["true"].copy()
    sol[0, 2, 1] = np.nan
    out, wout = fr.apply(c["tables"], sol, c["a1"], c["a2"], c["vis"])
    touched = (c["a1"] == 2) | (c["a2"] == 2)
    assert (wout[touched] == 0).all() and (wout[~touched] == 1).all() and np.array_equal(out[touched], c["vis"][touched])


COMPOSITION_BOUND = 5.2e-10  # measured 2.6e-10: the largest |average - 1| over the baselines after the correction


def test_composition_restores_the_averages():
    c = fc.composition_case()
    before = np.abs(c["vis"].mean(axis=(1, 2)))
    assert before.max() < 0.5  # measured 0.124
    sol, _, _, _ = fr.fringefit(c["tables"], c["vis"], c["a1"], c["a2"], c["A"], rounds=3, window_cells=(2, 2))
    out, _ = fr.apply(c["tables"], sol, c["a1"], c["a2"], c["vis"])
    after = np.abs(out.mean(axis=(1, 2)) - 1.0).max()
    print("composition", before.max(), after)
    assert after < COMPOSITION_BOUND
