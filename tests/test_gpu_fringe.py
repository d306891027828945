"""Delay and rate calibration on the device (gridhip_fringe_tables, gridhip_fringe_search, gridhip_fringe_solve,
gridhip_fringefit, gridhip_apply_fringe and their _dev forms) against the numpy restatement tests/fringe_ref.py.  The table
is compared within the rounding of the phasor recipe; given the library's table, the search and the solve are compared bit
for bit (np.array_equal): rounded products, sums in a fixed order and comparisons leave no tolerance to state.  The driver
runs with a general solution, whose derotation phasors differ by the rounding of sincospi: peak indices are equal and the
values stand within the project's bound for solvers, 1e-10.  The shapes are the smallest either side of the edges that
gridhip_fringe_tile() reports."""
import ctypes as C

import numpy as np
import pytest

import fringe_cases as fc
import fringe_ref as fr
from test_fringe_host import CLEAN_BOUNDS, COMPOSITION_BOUND, FLAGGED_BOUNDS
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the project's bound for solvers (gaincal, ddcal, dft_ref.TOL)


@pytest.fixture(scope="module")
def tile():
    import gridhip
    return gridhip.fringe_tile()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def dev(x):
    return None if x is None else to_dev(x)


def grid_axes(freq, time, tint, Nd, Nr):
    """Nd delays and Nr rates that span +-0.12 of the unambiguous ranges, a cell at zero where the count is odd"""
    tint, _ = fr.intervals(len(time), tint)
    dtau = 0.24 / (np.median(np.diff(freq)) if len(freq) > 1 else 1.0e6) / Nd
    drate = 0.24 / (np.median(np.diff(time)) if len(time) > 1 else 2.0) / Nr
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nr // 2) * drate, drate, Nr)


def search_case(B, T, F, tint, Nd, Nr, seed=0, specials=False):
    """a cube with one clear peak per baseline and interval, noise, a model and weights with flags"""
    rng = np.random.default_rng(seed)
    A = 6
    a1, a2 = fc.pairs(A)
    a1, a2 = a1[:B].copy(), a2[:B].copy()
    freq, time = fc.axes(T, F, jitter=0.2, seed=seed)
    _, I = fr.intervals(T, tint)
    true = fc.truth(A, I, freq, time, seed=seed + 1, frac=0.05)  # (the grids of these cases span +-0.12)
    model = rng.normal(size=(B, T, F)) + 1j * rng.normal(size=(B, T, F))
    vis = fc.corrupt(true, a1, a2, freq, time, tint) * model + 0.2 * (rng.normal(size=(B, T, F)) + 1j * rng.normal(size=(B, T, F)))
    wt = rng.uniform(0.5, 2.0, (B, T, F)) * (rng.uniform(size=(B, T, F)) > 0.15)
    if specials:
        vis[1] = 0.0               # all zero
        wt[2] = 0.0                # every sample flagged, NaN and Inf under zero weights
        vis[2, 0, 0], vis[2, T - 1, F - 1], wt[2, 1, 1] = np.nan, np.inf, np.nan
        vis[3, T // 2, F // 2] = np.nan  # one unflagged NaN
        wt[3, T // 2, F // 2] = 1.0
        a2[4] = a1[4]              # p == q
        a1[5] = A                  # out of range
        a2[6] = -1
    delays, rates = grid_axes(freq, time, tint, Nd, Nr)
    return dict(A=A, a1=a1, a2=a2, freq=freq, time=time, tint=tint, I=I, delays=delays, rates=rates, vis=vis, model=model,
                wt=wt, true=true)


def unit_sol(I, A, seed):
    """zero delays and rates (sincospi(0) is exact) and random unit phasors"""
    ph = np.random.default_rng(seed).uniform(-np.pi, np.pi, (I, A))
    sol = np.zeros((I, A, 4))
    sol[:, :, 2], sol[:, :, 3] = np.cos(ph), np.sin(ph)
    n = np.sqrt(sol[:, :, 2] ** 2 + sol[:, :, 3] ** 2)
    sol[:, :, 2], sol[:, :, 3] = sol[:, :, 2] / n, sol[:, :, 3] / n
    return sol


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,T,tint,Nd,Nr", [(1, 1, 0, 1, 1), (33, 8, 3, 9, 32), (16, 8, 0, 64, 32), (5, 7, 1, 3, 2)])
def test_tables(ctx, F, T, tint, Nd, Nr):
    freq, time = fc.axes(T, F, jitter=0.2)
    delays, rates = grid_axes(freq, time, tint, Nd, Nr)
    want = fr.tables(freq, time, tint, *delays, *rates)
    tab = ctx.fringe_tables(freq, time, tint, delays, rates)
    assert tab.shape == want.shape and tab[0] == 1.0
    assert np.array_equal(tab[:fr.HEAD], want[:fr.HEAD])
    assert np.abs(tab - want).max() <= 1e-13  # the bound test_gpu_rm.py uses for the same phasor recipe
    n = 2 * F * Nd + 2 * T * Nr
    assert np.array_equal(tab[fr.HEAD + n:], want[fr.HEAD + n:])  # tref, a, dt: plain differences
    assert same(host(ctx.fringe_tables(to_dev(freq), to_dev(time), tint, delays, rates)), tab), "the device form's bits"


def test_tables_judged_on_the_device(ctx):
    freq, time = fc.axes(4, 4)
    for f, t in ((np.array([1.0, np.nan, 3.0, 4.0]), time), (freq, np.array([0.0, 1.0, np.inf, 3.0]))):
        tab = ctx.fringe_tables(f, t, 0, (0.0, 1e-8, 4), (0.0, 0.1, 4))
        assert tab[0] == 0.0 and not tab[fr.HEAD:].any() and list(tab[1:7]) == [4, 4, 4, 1, 4, 4]


# ---- the search, bit for bit ---------------------------------------------------------------------------------------------------
def search_shapes(tile):
    tj, kc, tr = tile
    # B, T, F, tint, Nd, Nr, cells
    return [
        (15, 8, 4 * kc + 1, 0, tj + 1, tr, None),          # the largest: a tile + 1, chunks + 1
        (3, 4, kc - 1, 0, tj - 1, 3, None), (3, 4, kc, 0, tj, 3, None), (3, 4, kc + 1, 0, tj + 1, 3, None),
        (2, 3, 5, 0, 1, 4, None), (2, 3, 5, 0, 4, 1, None),  # Nd = 1; Nr = 1
        (2, 3, 5, 0, 3, tr - 1, None), (2, 3, 5, 0, 3, tr + 1, None),  # either side of a lane-pass of rates
        (3, 5, 6, 1, 5, 4, None),                           # tint = 1
        (3, 8, 6, 3, 5, 4, None),                           # tint does not divide T
        (1, 4, 9, 0, 2 * tj + 3, 5, None),                  # B = 1, three tiles
        (3, 4, 9, 0, 2 * tj + 3, 7, "edges"),               # sub-windows that put the peak on an edge
    ]


def run_search(ctx, c, sol, cells, tab):
    kw = dict(model_vis=c["model"], weights=c["wt"], sol=sol, cells=cells)
    args = (c["a1"], c["a2"], c["A"], c["tint"], c["delays"], c["rates"])
    want = fr.search(tab, c["vis"], c["a1"], c["a2"], c["A"], model=c["model"], wt=c["wt"], sol=sol, cells=cells)
    for run in range(2):
        got = ctx.fringe_search(c["vis"], tab, *args, **kw)
        assert same(got[0], want[0]) and same(got[1], want[1]), ("host", run, np.argwhere(got[0] != want[0])[:5])
    dkw = dict(model_vis=dev(c["model"]), weights=dev(c["wt"]), sol=dev(sol), cells=cells)
    dargs = (to_dev(c["a1"]), to_dev(c["a2"]), c["A"], c["tint"], c["delays"], c["rates"])
    for run in range(2):
        got = [host(x) for x in ctx.fringe_search(to_dev(c["vis"]), to_dev(tab), *dargs, **dkw)]
        assert same(got[0], want[0]) and same(got[1], want[1]), ("dev", run)
    return want


@pytest.mark.parametrize("index", range(12))
def test_search_bits(ctx, tile, index):
    B, T, F, tint, Nd, Nr, cells = search_shapes(tile)[index]
    c = search_case(B, T, F, tint, Nd, Nr, seed=index, specials=B == 15)
    tab = ctx.fringe_tables(c["freq"], c["time"], tint, c["delays"], c["rates"])
    whole = fr.search(tab, c["vis"], c["a1"], c["a2"], c["A"], model=c["model"], wt=c["wt"])[0]
    windows = [None]
    if cells == "edges":
        j, k = int(whole[0, 0, 0]), int(whole[0, 0, 1])
        assert 0 < j < Nd - 1 and 0 < k < Nr - 1, "the case must peak inside the grid"
        windows = [(j, Nd, k, Nr), (0, j + 1, 0, k + 1), (j, j + 1, k, k + 1), (j - 1, j + 2, k - 1, k + 2)]
    for cells in windows:
        for sol in (None, unit_sol(c["I"], c["A"], index)):
            want, stats = run_search(ctx, c, sol, cells, tab)
            assert stats[7] == 0
            if cells is not None and cells[0] == j and sol is None:  # on the lower edges: the grid values stand
                assert want[0, 0, 3] == c["delays"][0] + float(j) * c["delays"][1]
                assert want[0, 0, 4] == c["rates"][0] + float(k) * c["rates"][1]
    if B == 15:
        assert list(whole[1:7, 0, 10]) == [0, 1, 2, 3, 3, 3]
        assert list(whole[1, 0, :3]) == [0, 0, 0] and whole[1, 0, 7] == 0  # all zero: the tie goes to (j0, k0), coh2 = 0
        assert fr.weights(whole, c["a1"], c["a2"], c["A"], 0, 0.0, 0.0)[1] == 0  # ... and the baseline is excluded
        assert (whole[7:, 0, 10] == 0).all() and (whole[7:, 0, 7] > 0.2).all()


def test_search_refuses_what_does_not_fit(ctx):
    c = search_case(3, 4, 5, 0, 4, 3)
    tab = ctx.fringe_tables(c["freq"], c["time"], 0, c["delays"], c["rates"])
    peaks = np.full((3, 1, 12), 7.0)
    invalid, other_f, other_t = tab.copy(), tab.copy(), tab.copy()
    invalid[0], other_f[1], other_t[2] = 0.0, 6.0, 5.0  # valid = 0; a head of another F; of another T
    for t in (invalid, other_f, other_t):
        for form in (lambda x: x, to_dev):
            pk = form(peaks)
            got, stats = ctx.fringe_search(form(c["vis"]), form(t), form(c["a1"]), form(c["a2"]), c["A"], 0, c["delays"],
                                           c["rates"], peaks=pk)
            assert list(np.asarray(host(stats) if form is to_dev else stats)) == [0, 0, 0, 0, 0, 0, 0, 1]
            assert (np.asarray(host(pk) if form is to_dev else pk) == 7.0).all()
    # cells outside the table's grid: a table of 3 delays x 4 rates has the length of one of 4 x 3 when F == T
    c = search_case(3, 4, 4, 0, 3, 4)
    tab = ctx.fringe_tables(c["freq"], c["time"], 0, c["delays"], c["rates"])
    swapped = ((c["delays"][0], c["delays"][1], 4), (c["rates"][0], c["rates"][1], 3))
    for form in (lambda x: x, to_dev):
        pk = form(peaks)
        got, stats = ctx.fringe_search(form(c["vis"]), form(tab), form(c["a1"]), form(c["a2"]), c["A"], 0, *swapped, peaks=pk)
        assert list(np.asarray(host(stats) if form is to_dev else stats)) == [0, 0, 0, 0, 0, 0, 0, 1]
        assert (np.asarray(host(pk) if form is to_dev else pk) == 7.0).all()


def test_a_table_of_another_tint_is_refused(ctx):
    """peaks and sol are sized by the caller's tint; the table's head says how many intervals the kernels walk.  A numpy
    table is compared in the binding and raises; on the device the kernels refuse and touch nothing."""
    c = search_case(3, 8, 5, 2, 4, 3)  # made with tint = 2: four intervals
    tab = ctx.fringe_tables(c["freq"], c["time"], 2, c["delays"], c["rates"])
    args = (c["a1"], c["a2"], c["A"])
    for tint in (0, 4, 1):  # one, two and eight intervals
        with pytest.raises(ValueError):
            ctx.fringe_search(c["vis"], tab, *args, tint, c["delays"], c["rates"])
        with pytest.raises(ValueError):
            ctx.apply_fringe(np.zeros((fr.intervals(8, tint)[1], c["A"], 4)), tab, c["vis"], c["a1"], c["a2"], tint)
        I = fr.intervals(8, tint)[1]
        dargs = (to_dev(c["a1"]), to_dev(c["a2"]), c["A"])
        pk = to_dev(np.full((3, I, 12), 7.0))
        sol = to_dev(unit_sol(I, c["A"], 3))
        got, stats = ctx.fringe_search(to_dev(c["vis"]), to_dev(tab), *dargs, tint, c["delays"], c["rates"], sol=sol, peaks=pk)
        assert list(host(stats)) == [0, 0, 0, 0, 0, 0, 0, 1] and (host(pk) == 7.0).all()
        out, wout = to_dev(np.full(c["vis"].shape, 5 + 1j)), to_dev(np.full(c["vis"].shape, 3.0))
        ctx.apply_fringe(sol, to_dev(tab), to_dev(c["vis"]), dargs[0], dargs[1], tint, out=out, weights_out=wout)
        assert (host(out) == 5 + 1j).all() and (host(wout) == 3.0).all()
    # the C ABI's host form with a wrong I: refused by the kernels, the arrays as they were
    from gridhip import _lib
    lib, ptr = _lib.load(), lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    vis, a1, a2 = np.ascontiguousarray(c["vis"]), np.ascontiguousarray(c["a1"]), np.ascontiguousarray(c["a2"])
    pk, st = np.full((3, 1, 12), 7.0), np.zeros(8)
    assert lib.gridhip_fringe_search(ctx._h, 3, 8, 5, c["A"], 1, ptr(tab), ptr(vis), None, None, ptr(a1), ptr(a2), None, 0, 4, 0,
                                     3, ptr(pk), ptr(st)) == 0
    assert list(st) == [0, 0, 0, 0, 0, 0, 0, 1] and (pk == 7.0).all()
    sol, out = unit_sol(1, c["A"], 3), np.full(vis.shape, 5 + 1j)
    assert lib.gridhip_apply_fringe(ctx._h, 3, 8, 5, c["A"], 1, ptr(tab), ptr(sol), ptr(a1), ptr(a2), 1, ptr(vis), None, ptr(out),
                                    None) == 0
    assert (out == 5 + 1j).all()


# ---- the solve, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solve_peaks():
    c = search_case(15, 8, 9, 4, 9, 8, seed=21)
    tab = fr.tables(c["freq"], c["time"], 4, *c["delays"], *c["rates"])
    peaks, _ = fr.search(tab, c["vis"], c["a1"], c["a2"], c["A"], model=c["model"], wt=c["wt"])
    assert (peaks[:, :, 10] == 0).all()
    touches4 = (c["a1"] == 4) | (c["a2"] == 4)
    peaks[touches4, 1, 10] = 2.0      # interval 1: antenna 4 has no usable baseline
    peaks[0, 0, 7] = 0.01             # interval 0: min_coh2 cuts baseline 0
    peaks[1, 0, 8] = 3.0              # ... and min_count baseline 1
    peaks.setflags(write=False)
    return c, peaks


@pytest.mark.parametrize("refant,niter,tol", [(0, 50, 0.0), (4, 50, 1e-9), (None, 7, 0.0), (2, 0, 0.0)])
def test_solve_bits(ctx, solve_peaks, refant, niter, tol):
    c, peaks = solve_peaks
    A = c["A"]
    sol0 = fc.truth(A, 2, c["freq"], c["time"], seed=8)
    kw = dict(min_count=10, min_coh2=0.05, refant=refant, niter=niter, tol=tol)
    want = fr.solve(peaks, c["a1"], c["a2"], A, sol0, **kw)
    assert want[1][1, 4] == 0 and want[2][2] == 1 and want[2][1] == 15 + 10 - 2
    assert want[2][3] == (1 if refant == 4 else 0)  # an unsolved refant leaves its interval unreferenced
    assert np.array_equal(want[0][1, 4], sol0[1, 4])  # the unsolved antenna keeps its very bits
    for run in range(2):
        got = ctx.fringe_solve(np.array(peaks), c["a1"], c["a2"], A, sol=sol0.copy(), **kw)
        assert all(same(g, w) for g, w in zip(got, want)), ("host", run, got[2], want[2])
        got = ctx.fringe_solve(to_dev(np.array(peaks)), to_dev(c["a1"]), to_dev(c["a2"]), A, sol=to_dev(sol0), **kw)
        assert all(same(host(g), w) for g, w in zip(got, want)), ("dev", run)
    cold = ctx.fringe_solve(np.array(peaks), c["a1"], c["a2"], A, **kw)
    cold_want = fr.solve(peaks, c["a1"], c["a2"], A, np.tile([0.0, 0.0, 1.0, 0.0], (2, A, 1)), **kw)
    assert all(same(g, w) for g, w in zip(cold, cold_want))


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def fit_close(got, want, delays, rates):
    sol, peaks, info, stats = got
    wsol, wpeaks, winfo, wstats = want
    assert np.array_equal(peaks[..., [0, 1, 8, 10]], wpeaks[..., [0, 1, 8, 10]]) and np.array_equal(info, winfo)
    assert np.abs(sol[..., 0] - wsol[..., 0]).max() <= TOL * delays[1] and np.abs(sol[..., 1] - wsol[..., 1]).max() <= TOL * rates[1]
    assert np.abs(sol[..., 2:] - wsol[..., 2:]).max() <= TOL
    assert np.abs(peaks[..., 3] - wpeaks[..., 3]).max() <= TOL * delays[1]
    assert np.abs(peaks[..., 4] - wpeaks[..., 4]).max() <= TOL * rates[1]
    assert np.abs(peaks[..., 5:8] - wpeaks[..., 5:8]).max() <= TOL
    assert np.array_equal(stats[[1, 2, 3, 4, 7]], wstats[[1, 2, 3, 4, 7]])


@pytest.mark.parametrize("flag_fraction,bounds", [(0.0, CLEAN_BOUNDS), (0.3, FLAGGED_BOUNDS)])
def test_fringefit_three_rounds(ctx, flag_fraction, bounds):
    c = fc.recovery_case(flag_fraction)
    A = c["A"]
    tab = ctx.fringe_tables(c["freq"], c["time"], 0, c["delays"], c["rates"])
    kw = dict(rounds=3, window=(2, 2), refant=0, niter=50)
    # a general solution to start from: a tenth of the truth's delays and rates off, random phasors
    start = fc.truth(A, 1, c["freq"], c["time"], seed=31, frac=0.005)
    for sol0 in (None, start):
        want = fr.fringefit(tab, c["vis"], c["a1"], c["a2"], A, wt=c["wt"], sol=None if sol0 is None else sol0.copy(),
                            rounds=3, window_cells=(2, 2), refant=0, niter=50)
        got = ctx.fringefit(c["vis"], tab, c["a1"], c["a2"], A, 0, c["delays"], c["rates"], weights=c["wt"],
                            sol=None if sol0 is None else sol0.copy(), **kw)
        fit_close(got, want, c["delays"], c["rates"])
        dgot = ctx.fringefit(to_dev(c["vis"]), to_dev(tab), to_dev(c["a1"]), to_dev(c["a2"]), A, 0, c["delays"], c["rates"],
                             weights=dev(c["wt"]), sol=dev(sol0), **kw)
        assert all(same(host(d), g) for d, g in zip(dgot, got)), "host and device forms: the same bits"
        err = fc.errors(got[0], c["true"], c["delays"], c["rates"])
        print("fringefit", flag_fraction, sol0 is not None, err)
        if sol0 is None:  # the truth bounds of the host test hold for the device's result
            assert err[0] < bounds[1][0] and err[1] < bounds[1][1]
    one = ctx.fringefit(c["vis"], tab, c["a1"], c["a2"], A, 0, c["delays"], c["rates"], weights=c["wt"], rounds=1, refant=0)
    err = fc.errors(one[0], c["true"], c["delays"], c["rates"])
    assert err[0] < bounds[0][0] and err[1] < bounds[0][1]


# ---- apply ------------------------------------------------------------------------------------------------------------------------
def test_apply_fringe(ctx):
    c = search_case(15, 8, 9, 3, 4, 4, seed=41)
    A, a1, a2, vis, wt = c["A"], fc.pairs(6)[0], fc.pairs(6)[1], c["vis"], c["wt"]
    tab = ctx.fringe_tables(c["freq"], c["time"], 3, c["delays"], c["rates"])
    sol = c["true"]
    bound = 4e-13 * np.abs(vis)  # three table-recipe phasors and a product
    for inverse in (True, False):
        want, wwant = fr.apply(tab, sol, a1, a2, vis, wt, inverse=inverse)
        out, wout = ctx.apply_fringe(sol, tab, vis, a1, a2, 3, inverse=inverse, weights=wt)
        assert (np.abs(out - want) <= bound).all() and np.array_equal(wout, wt)
        dout, dwout = ctx.apply_fringe(to_dev(sol), to_dev(tab), to_dev(vis), to_dev(a1), to_dev(a2), 3, inverse=inverse,
                                       weights=to_dev(wt))
        assert same(host(dout), out) and same(host(dwout), wout)
    fwd, _ = ctx.apply_fringe(sol, tab, vis, a1, a2, 3, inverse=False)
    back, ones = ctx.apply_fringe(sol, tab, fwd, a1, a2, 3, inverse=True)
    assert (np.abs(back - vis) <= bound).all() and (ones == 1.0).all()
    # a NaN row, an antenna out of range: the value is kept, the weight is +0.0
    bad, b1 = sol.copy(), a1.copy()
    bad[1, 2, 0] = np.nan
    b1[0] = 6
    out, wout = ctx.apply_fringe(bad, tab, vis, b1, a2, 3, weights=wt)
    hit = np.zeros(vis.shape, dtype=bool)
    hit[(b1 == 2) | (a2 == 2), 3:6] = True
    hit[0] = True
    assert np.array_equal(out[hit], vis[hit]) and not wout[hit].any() and not np.signbit(wout[hit]).any()
    assert np.array_equal(wout[~hit], wt[~hit]) and (np.abs(out - fr.apply(tab, sol, a1, a2, vis)[0])[~hit] <= bound[~hit]).all()
    # in place
    want, _ = ctx.apply_fringe(sol, tab, vis, a1, a2, 3, weights=wt)
    v, w = vis.copy(), wt.copy()
    ctx.apply_fringe(sol, tab, v, a1, a2, 3, weights=w, out=v, weights_out=w)
    assert same(v, want) and same(w, wt)
    dv, dw = to_dev(vis), to_dev(wt)
    ctx.apply_fringe(to_dev(sol), to_dev(tab), dv, to_dev(a1), to_dev(a2), 3, weights=dw, out=dv, weights_out=dw)
    assert same(host(dv), want) and same(host(dw), wt)


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_composition_restores_the_averages(ctx):
    c = fc.composition_case()
    tab = ctx.fringe_tables(c["freq"], c["time"], 0, c["delays"], c["rates"])
    before = np.abs(c["vis"].mean(axis=(1, 2)))
    sol, _, info, stats = ctx.fringefit(c["vis"], tab, c["a1"], c["a2"], c["A"], 0, c["delays"], c["rates"], rounds=3)
    out, _ = ctx.apply_fringe(sol, tab, c["vis"], c["a1"], c["a2"], 0)
    after = np.abs(out.mean(axis=(1, 2)) - 1.0)
    print("composition", before.max(), after.max())
    assert before.max() < 0.5 and after.max() < COMPOSITION_BOUND and stats[4] == 0 and stats[7] == 0


def test_a_captured_chain_replays_to_the_eager_result(ctx):
    import torch
    c = fc.recovery_case(0.3)
    A = c["A"]
    tab = ctx.fringe_tables(c["freq"], c["time"], 0, c["delays"], c["rates"])
    dv, dw, dt, d1, d2 = to_dev(c["vis"]), to_dev(c["wt"]), to_dev(tab), to_dev(c["a1"]), to_dev(c["a2"])
    out, wout = torch.empty_like(dv), torch.empty_like(dw)

    def chain():
        fit = ctx.fringefit(dv, dt, d1, d2, A, 0, c["delays"], c["rates"], weights=dw, rounds=3, niter=50)
        return fit + ctx.apply_fringe(fit[0], dt, dv, d1, d2, 0, weights=dw, out=out, weights_out=wout)

    want = [host(x).copy() for x in chain()]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds the scratch
        chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        res = chain()
    torch.cuda.synchronize()
    for _ in range(2):
        for x in res:
            x.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(host(x), w) for x, w in zip(res, want))


# ---- the rules ----------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header through the C ABI on device memory, and the arrays as they were given."""
    import torch
    from gridhip import _lib
    lib, h = _lib.load(), ctx._h
    B, T, F, A, Nd, Nr, I = 3, 4, 5, 3, 6, 4, 2
    nt = fr.table_doubles(F, T, Nd, Nr)
    full = lambda m, val, dt=torch.float64: torch.full((m,), val, dtype=dt, device="cuda:0")  # noqa: E731
    n = B * T * F
    t = dict(f=full(F, 1.0), t=full(T, 2.0), tab=full(nt, 7.0), v=full(n, 3 + 4j, torch.complex128),
             m=full(n, 1 - 1j, torch.complex128), w=full(n, 1.0), a1=full(B, 0, torch.int64), a2=full(B, 1, torch.int64),
             sol=full(I * A * 4, 0.5), pk=full(B * I * 12, 5.0), info=full(I * A, 4.0), s=full(8, 6.0),
             o=full(n, 8 + 0j, torch.complex128), wo=full(n, 9.0))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    NAN, INF = np.nan, np.inf

    def tb(F=F, T=T, tint=2, f=p["f"], tm=p["t"], Nd=Nd, Nr=Nr, tab=p["tab"]):
        return lib.gridhip_fringe_tables_dev(h, F, T, tint, f, tm, -1.0, 0.5, Nd, -1.0, 0.5, Nr, tab)

    def se(B=B, T=T, F=F, A=A, I=I, tab=p["tab"], v=p["v"], m=p["m"], w=p["w"], a1=p["a1"], a2=p["a2"], sol=p["sol"], j0=0, j1=Nd,
           k0=0, k1=Nr, pk=p["pk"], s=p["s"]):
        return lib.gridhip_fringe_search_dev(h, B, T, F, A, I, tab, v, m, w, a1, a2, sol, j0, j1, k0, k1, pk, s)

    def so(B=B, I=I, A=A, a1=p["a1"], a2=p["a2"], pk=p["pk"], mc=0.0, mh=0.0, ref=0, niter=5, tol=0.0, sol=p["sol"],
           info=p["info"], s=p["s"]):
        return lib.gridhip_fringe_solve_dev(h, B, I, A, a1, a2, pk, mc, mh, ref, niter, tol, sol, info, s)

    def ff(I=I, Nd=Nd, Nr=Nr, tab=p["tab"], v=p["v"], rounds=2, wj=1, wk=1, warm=0, sol=p["sol"], pk=p["pk"], info=p["info"],
           s=p["s"], niter=5, ref=0):
        return lib.gridhip_fringefit_dev(h, B, T, F, A, I, Nd, Nr, tab, v, p["m"], p["w"], p["a1"], p["a2"], rounds, wj, wk, 0.0,
                                         0.0, ref, niter, 0.0, warm, sol, pk, info, s)

    def ap(F=F, A=A, I=I, tab=p["tab"], sol=p["sol"], a1=p["a1"], inverse=1, v=p["v"], w=p["w"], o=p["o"], wo=p["wo"]):
        return lib.gridhip_apply_fringe_dev(h, B, T, F, A, I, tab, sol, a1, p["a2"], inverse, v, w, o, wo)

    bad = [tb(F=0), tb(F=1025), tb(T=0), tb(tint=-1), tb(tint=257, T=300), tb(T=257, tint=0), tb(Nd=0), tb(Nd=4097), tb(Nr=0),
           tb(Nr=1025), tb(f=None), tb(tm=None), tb(tab=None), tb(tab=p["f"]), tb(tm=at("tab", 8 * (nt - 1))),
           se(B=0), se(T=0), se(F=0), se(F=1025), se(A=1), se(I=0), se(I=5), se(tab=None), se(v=None), se(a1=None), se(a2=None), se(pk=None),
           se(s=None), se(j0=-1), se(j0=2, j1=2), se(j1=4097), se(k0=-1), se(k0=3, k1=3), se(k1=1025), se(v=at("v", 8)),
           se(m=at("m", 8)), se(pk=p["v"]), se(pk=p["sol"]), se(s=p["w"]), se(s=at("pk", 0)), se(pk=at("tab", 0)),
           so(B=0), so(I=0), so(A=1), so(a1=None), so(a2=None), so(pk=None), so(sol=None), so(info=None), so(s=None), so(mc=-1.0),
           so(mc=NAN), so(mh=-0.5), so(mh=INF), so(ref=3), so(niter=-1), so(niter=100001), so(tol=-1.0), so(tol=NAN),
           so(sol=p["pk"]), so(info=p["sol"]), so(s=at("info", 0)),
           ff(I=0), ff(I=5), ff(Nd=0), ff(Nd=4097), ff(Nr=0), ff(Nr=1025), ff(rounds=0), ff(rounds=5), ff(wj=-1), ff(wj=4097),
           ff(wk=-1), ff(wk=1025), ff(warm=2), ff(tab=None), ff(v=None), ff(sol=None), ff(pk=None), ff(info=None), ff(s=None),
           ff(niter=-1), ff(ref=3), ff(sol=p["pk"]), ff(pk=p["v"]), ff(info=at("sol", 0)),
           ap(F=0), ap(F=1025), ap(A=1), ap(I=0), ap(I=5), ap(tab=None), ap(sol=None), ap(a1=None), ap(v=None), ap(o=None), ap(inverse=2),
           ap(inverse=-1), ap(v=at("v", 8)), ap(o=at("o", 8)), ap(o=at("v", 16)), ap(wo=at("w", 8)), ap(o=p["m"], wo=p["m"]),
           ap(wo=p["sol"]), ap(o=at("tab", 0))]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), [i for i, rc in enumerate(bad) if rc != _lib.EINVAL]
    assert lib.gridhip_fringe_tile(None) == _lib.EINVAL
    assert so(A=1025) == _lib.EUNSUPPORTED and se(A=1025) == _lib.EUNSUPPORTED
    for fn, args in ((lib.gridhip_fringe_tables_dev, (F, T, 2, p["f"], p["t"], -1.0, 0.5, Nd, -1.0, 0.5, Nr, p["tab"])),
                     (lib.gridhip_fringe_solve_dev, (B, I, A, p["a1"], p["a2"], p["pk"], 0.0, 0.0, 0, 5, 0.0, p["sol"], p["info"], p["s"])),
                     (lib.gridhip_apply_fringe_dev, (B, T, F, A, I, p["tab"], p["sol"], p["a1"], p["a2"], 1, p["v"], p["w"], p["o"], p["wo"]))):
        assert fn(None, *args) == _lib.EINVAL
    torch.cuda.synchronize()
    for key, val in (("f", 1.0), ("t", 2.0), ("tab", 7.0), ("v", 3 + 4j), ("m", 1 - 1j), ("w", 1.0), ("sol", 0.5), ("pk", 5.0),
                     ("info", 4.0), ("s", 6.0), ("o", 8 + 0j), ("wo", 9.0)):
        assert bool((t[key] == val).all()), key
    # a table that is not one (its head holds 7.0): stats[7] = 1 and the sentinels stay
    assert se() == 0 and bool((t["pk"] == 5.0).all()) and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    t["s"].fill_(6.0)
    assert ff() == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1]) and bool((t["pk"] == 5.0).all())
    assert ap() == 0 and bool((t["o"] == 8 + 0j).all()) and bool((t["wo"] == 9.0).all())
    # in place is no overlap
    assert tb() == 0 and ap(o=p["v"], wo=p["w"]) == 0
    torch.cuda.synchronize()
