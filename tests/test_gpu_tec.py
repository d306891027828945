"""Dispersive delay (TEC) calibration on the device (gridhip_tec_tables, gridhip_tec_search, gridhip_tecfit, gridhip_apply_tec
and their _dev forms) against the numpy restatement tests/tec_ref.py.  The table's phasors are compared within the rounding
of sincospi, its head, a, c and s bit for bit; given the library's table, the search is compared bit for bit
(np.array_equal): rounded products, sums in a fixed order and comparisons leave no tolerance to state.  The driver runs
with a general solution, whose derotation phasors differ by the rounding of sincospi: peak indices are equal and the values
stand within the project's bound for solvers, 1e-10 of a cell.  The shapes are the smallest either side of the edges that
gridhip_tec_tile() reports."""
import ctypes as C

import numpy as np
import pytest

import tec_cases as tc
import tec_ref as tr
from test_gpu_imager import host, to_dev
from test_tec_host import CLEAN_BOUNDS, COMPOSITION_BOUND, COMPOSITION_ROUNDS, FLAGGED_BOUNDS

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the project's bound for solvers (gaincal, ddcal, the fringe driver)


@pytest.fixture(scope="module")
def tile():
    import gridhip
    return gridhip.tec_tile()


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def dev(x):
    return None if x is None else to_dev(x)


def grid_axes(freq, Nd, Nm):
    """Nd delays that span +-0.12 of the unambiguous range and Nm TEC cells that span +-0.3 TEC units, a cell at zero where
    the count is odd"""
    dtau = 0.24 / (np.median(np.diff(freq)) if len(freq) > 1 else 1.0e6) / Nd
    dtec = 0.6 / Nm
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nm // 2) * dtec, dtec, Nm)


def search_case(F, Nd, Nm, seed=0, A=3, T=3, tint=2):
    """a cube with one clear peak per baseline and interval, noise, a model and weights with 20 % zeros and a NaN under one"""
    rng = np.random.default_rng(seed)
    a1, a2 = tc.pairs(A)
    B = len(a1)
    freq = tc.band(F, jitter=0.2, seed=seed)
    _, I = tr.intervals(T, tint)
    true = tc.truth(A, I, freq, seed=seed + 1, frac=0.05, tec_max=0.1)  # (the grids of these cases span +-0.12, +-0.3)
    model = rng.normal(size=(B, T, F)) + 1j * rng.normal(size=(B, T, F))
    vis = tc.corrupt(true, a1, a2, freq, T, tint) * model + 0.2 * (rng.normal(size=(B, T, F)) + 1j * rng.normal(size=(B, T, F)))
    wt = rng.uniform(0.5, 2.0, (B, T, F)) * (rng.uniform(size=(B, T, F)) > 0.2)
    wt[B - 1, T - 1, F - 1] = 0.0
    vis_nan = vis.copy()
    vis_nan[B - 1, T - 1, F - 1] = np.nan  # under a zero weight: ignored (only ever passed with the weights)
    delays, tecs = grid_axes(freq, Nd, Nm)
    return dict(A=A, T=T, a1=a1, a2=a2, freq=freq, tint=tint, I=I, delays=delays, tecs=tecs, vis=vis, vis_nan=vis_nan,
                model=model, wt=wt, true=true)


def unit_sol(I, A, seed):
    """zero delays and TEC (sincospi(0) is exact) and random unit phasors"""
    ph = np.random.default_rng(seed).uniform(-np.pi, np.pi, (I, A))
    sol = np.zeros((I, A, 4))
    sol[:, :, 2], sol[:, :, 3] = np.cos(ph), np.sin(ph)
    n = np.sqrt(sol[:, :, 2] ** 2 + sol[:, :, 3] ** 2)
    sol[:, :, 2], sol[:, :, 3] = sol[:, :, 2] / n, sol[:, :, 3] / n
    return sol


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 17])
def test_tables(ctx, tile, F):
    tj, tm, _ = tile
    freq = tc.band(F, jitter=0.2)
    for Nd in (1, tj - 1, tj + 1):
        for Nm in (1, tm - 1, tm + 1):
            delays, tecs = grid_axes(freq, Nd, Nm)
            want = tr.tables(freq, 5, 2, *delays, *tecs)
            tab = ctx.tec_tables(freq, 5, 2, delays, tecs)
            assert tab.shape == want.shape and tab[0] == 1.0
            assert np.array_equal(tab[:tr.HEAD], want[:tr.HEAD])  # the head, with s
            assert np.abs(tab - want).max() <= 1e-13  # the bound test_gpu_rm.py uses for the same phasor recipe
            n = 2 * F * Nd + 2 * F * Nm
            assert np.array_equal(tab[tr.HEAD + n:], want[tr.HEAD + n:])  # a, c: rounded operations only
            assert same(host(ctx.tec_tables(to_dev(freq), 5, 2, delays, tecs)), tab), "the device form's bits"
    assert ctx.tec_tables(freq, 300, 0, (0.0, 1e-9, 2), (0.0, 0.1, 2))[3] == 300  # no cap of 256 on tint


def test_tables_judged_on_the_device(ctx):
    good = tc.band(4)
    for f, tecs in ((np.array([1.2e8, np.nan, 1.6e8, 1.8e8]), (0.0, 0.1, 4)), (np.array([1.2e8, 0.0, 1.6e8, 1.8e8]), (0.0, 0.1, 4)),
                    (np.array([-1.2e8, 1.4e8, 1.6e8, 1.8e8]), (0.0, 0.1, 4))):
        tab = ctx.tec_tables(f, 4, 0, (0.0, 1e-8, 4), tecs)
        assert tab[0] == 0.0 and not tab[tr.HEAD:].any() and list(tab[1:7]) == [4, 4, 4, 1, 4, 4] and list(tab[11:13]) == [0, 0]
        assert same(tab, tr.tables(f, 4, 0, 0.0, 1e-8, 4, *tecs))
    # dtec <= 0: the binding refuses it, so through the C ABI
    from gridhip import _lib
    lib = _lib.load()
    for dtec in (0.0, -0.1):
        tab = np.full(tr.table_doubles(4, 4, 4), 7.0)
        assert lib.gridhip_tec_tables(ctx._h, 4, 4, 0, C.c_void_p(good.ctypes.data), 0.0, 1e-8, 4, 0.0, dtec, 4,
                                      C.c_void_p(tab.ctypes.data)) == 0
        assert same(tab, tr.tables(good, 4, 0, 0.0, 1e-8, 4, 0.0, dtec, 4)) and tab[0] == 0.0 and not tab[tr.HEAD:].any()


# ---- the search, bit for bit ---------------------------------------------------------------------------------------------------
def grids(tile):
    tj, tm, _ = tile
    return [(1, 1), (tj - 1, tm + 1), (tj + 1, tm - 1), (2 * tj + 1, 1)]


def channels(tile):
    kc = tile[2]
    return [1, kc - 1, kc, kc + 1, 2 * kc + 1]


def run_search(ctx, c, tab, model, wt, sol, cells):
    vis = c["vis"] if wt is None else c["vis_nan"]
    want = tr.search(tab, vis, c["a1"], c["a2"], c["A"], model=model, wt=wt, sol=sol, cells=cells)
    args = (c["a1"], c["a2"], c["A"], c["tint"], c["delays"], c["tecs"])
    for run in range(2):
        got = ctx.tec_search(vis, tab, *args, model_vis=model, weights=wt, sol=sol, cells=cells)
        assert same(got[0], want[0]) and same(got[1], want[1]), ("host", run, np.argwhere(got[0] != want[0])[:5])
    dargs = (to_dev(c["a1"]), to_dev(c["a2"]), c["A"], c["tint"], c["delays"], c["tecs"])
    got = [host(x) for x in ctx.tec_search(to_dev(vis), to_dev(tab), *dargs, model_vis=dev(model), weights=dev(wt), sol=dev(sol),
                                           cells=cells)]
    assert same(got[0], want[0]) and same(got[1], want[1]), "dev"
    return want


@pytest.mark.parametrize("fi", range(5))
@pytest.mark.parametrize("gi", range(4))
def test_search_bits(ctx, tile, gi, fi):
    F, (Nd, Nm) = channels(tile)[fi], grids(tile)[gi]
    c = search_case(F, Nd, Nm, seed=5 * gi + fi)
    assert (c["a1"].size, c["T"], c["I"]) == (3, 3, 2)  # B = 3, the last interval short
    tab = ctx.tec_tables(c["freq"], c["T"], c["tint"], c["delays"], c["tecs"])
    windows = [None]
    if Nd > 1:
        windows.append((Nd // 3, Nd, Nm // 3, Nm))  # a window whose tiles start elsewhere and cut the grid's
    sol = unit_sol(c["I"], c["A"], gi)
    for cells in windows:
        for model, wt, s in ((None, None, None), (c["model"], c["wt"], None), (c["model"], c["wt"], sol)):
            peaks, stats = run_search(ctx, c, tab, model, wt, s, cells)
            assert stats[7] == 0 and stats[1] == 0 and stats[2] + stats[4] == 6  # (one channel: a flagged interval is empty)
            assert stats[0] == (0 if wt is None else (wt == 0).sum())
            if wt is None:
                assert stats[4] == 6 and (peaks[:, :, 10] == 0).all()


@pytest.mark.parametrize("Nd,Nm", [(5, 3), (65, 2)])
def test_search_bits_of_narrow_tiles(ctx, tile, Nd, Nm):
    """a tile of few delays stages more channels at a time - tile_j * chunk entries in rows of the delays rounded up to 64:
    F either side of that chunk and of two of them"""
    tj, _, kc = tile
    cap = (tj * kc) // (-(-Nd // 64) * 64)
    assert cap > kc
    for F in (cap - 1, cap, cap + 1, 2 * cap + 1):
        c = search_case(F, Nd, Nm, seed=F)
        tab = ctx.tec_tables(c["freq"], c["T"], c["tint"], c["delays"], c["tecs"])
        for model, wt, s in ((None, None, None), (c["model"], c["wt"], unit_sol(c["I"], c["A"], F))):
            run_search(ctx, c, tab, model, wt, s, None)
            run_search(ctx, c, tab, model, wt, s, (1, Nd - 1, 0, Nm - 1))


@pytest.mark.parametrize("T,tint", [(130, 0), (130, 70), (257, 0)])
def test_search_bits_of_long_intervals(ctx, T, tint):
    """tint has no cap of 256: intervals longer than the 64 time steps the refinement's energy takes per pass, a last pass
    that is short, and one of 257 steps"""
    c = search_case(3, 5, 3, seed=T + tint, T=T, tint=tint)
    tab = ctx.tec_tables(c["freq"], T, tint, c["delays"], c["tecs"])
    for model, wt, s in ((None, None, None), (c["model"], c["wt"], unit_sol(c["I"], c["A"], T))):
        peaks, stats = run_search(ctx, c, tab, model, wt, s, None)
        assert stats[7] == 0 and stats[4] == 3 * c["I"]


def border_case(tile, which):
    """one baseline whose true effective delay and TEC lie on the cell (tile_j - 1, tile_m - 1), the last of a tile on both
    axes (which = 0), or on (tile_j, tile_m), the first of the next (which = 1)"""
    tj, tm, _ = tile
    F, T, A = 9, 2, 2
    freq = tc.band(F)
    Nd, Nm = 2 * tj, 2 * tm
    dtau, dtec = 0.24 / np.median(np.diff(freq)) / Nd, 0.8 / Nm
    delays, tecs = (-(Nd // 2 - 3) * dtau, dtau, Nd), (-(Nm // 2 - 1) * dtec, dtec, Nm)
    j, m = tj - 1 + which, tm - 1 + which
    tau, tec = delays[0] + j * dtau, tecs[0] + m * dtec
    _, _, _, s = tr.coordinates(freq)
    true = (np.array([[tau - s * tec, 0.0]]), np.array([[tec, 0.0]]), np.array([[0.4, 0.0]]))
    a1, a2 = np.array([0], dtype=np.int64), np.array([1], dtype=np.int64)
    return dict(A=A, T=T, a1=a1, a2=a2, freq=freq, tint=0, delays=delays, tecs=tecs, j=j, m=m,
                vis=tc.corrupt(true, a1, a2, freq, T, 0))


@pytest.mark.parametrize("which", [0, 1])
def test_peak_across_a_tile_border(ctx, tile, which):
    c = border_case(tile, which)
    tab = ctx.tec_tables(c["freq"], c["T"], 0, c["delays"], c["tecs"])
    want, wstats = tr.search(tab, c["vis"], c["a1"], c["a2"], c["A"])
    assert (want[0, 0, 0], want[0, 0, 1]) == (c["j"], c["m"]) and want[0, 0, 10] == 0, "the case must peak on the border cell"
    assert abs(want[0, 0, 3] - (c["delays"][0] + c["j"] * c["delays"][1])) < 0.01 * c["delays"][1]  # both parabolas ran and
    assert abs(want[0, 0, 4] - (c["tecs"][0] + c["m"] * c["tecs"][1])) < 0.01 * c["tecs"][1]        # found the cell's centre
    got = ctx.tec_search(c["vis"], tab, c["a1"], c["a2"], c["A"], 0, c["delays"], c["tecs"])
    assert same(got[0], want) and same(got[1], wstats)


def test_an_exact_tie_across_tiles(ctx, tile):
    """all-zero visibilities under unit weights: every cell's power is 0, so the reduction within a tile and the refinement's
    choice among the four tiles are decided by the tie rule alone - the lowest delay, then the lowest TEC cell - on the
    whole grid and on a window that starts one cell in on both axes"""
    tj, tm, _ = tile
    F, T, A = 3, 2, 2
    Nd, Nm = tj + 1, tm + 1
    freq = tc.band(F)
    delays, tecs = grid_axes(freq, Nd, Nm)
    a1, a2 = np.array([0], dtype=np.int64), np.array([1], dtype=np.int64)
    vis, wt = np.zeros((1, T, F), dtype=np.complex128), np.ones((1, T, F))
    tab = ctx.tec_tables(freq, T, 0, delays, tecs)
    for cells, peak in ((None, (0, 0)), ((1, Nd, 1, Nm), (1, 1))):
        want, wstats = tr.search(tab, vis, a1, a2, A, wt=wt, cells=cells)
        got = ctx.tec_search(vis, tab, a1, a2, A, 0, delays, tecs, weights=wt, cells=cells)
        assert same(got[0], want) and same(got[1], wstats)
        row = got[0][0, 0]
        assert (row[0], row[1]) == peak and row[7] == 0 and row[10] == 0, "the peak, coh^2 and the class"


def test_search_classes(ctx):
    c = search_case(5, 6, 4, seed=3, A=6, T=4, tint=0)
    vis, wt, a1, a2 = c["vis"].copy(), np.ones(c["vis"].shape), c["a1"].copy(), c["a2"].copy()
    vis[1] = 0.0
    wt[2] = 0.0
    vis[2, 3, 4] = np.nan
    vis[3, 1, 2] = np.nan
    a2[4] = a1[4]
    a1[5] = 99
    tab = ctx.tec_tables(c["freq"], 4, 0, c["delays"], c["tecs"])
    want = tr.search(tab, vis, a1, a2, c["A"], wt=wt, cells=(1, 5, 1, 4))
    assert list(want[0][:6, 0, 10]) == [0, 0, 1, 2, 3, 3] and list(want[0][1, 0, :3]) == [1, 1, 0] and want[0][1, 0, 7] == 0
    for form in (lambda x: x, to_dev):
        got = ctx.tec_search(form(vis), form(tab), form(a1), form(a2), c["A"], 0, c["delays"], c["tecs"], weights=form(wt),
                             cells=(1, 5, 1, 4))
        got = [np.asarray(host(g) if form is to_dev else g) for g in got]
        assert same(got[0], want[0]) and same(got[1], want[1])


def test_search_refuses_what_does_not_fit(ctx):
    c = search_case(5, 4, 3, seed=2, T=4)
    tab = ctx.tec_tables(c["freq"], 4, 2, c["delays"], c["tecs"])
    args, vis4 = (c["a1"], c["a2"], c["A"]), c["vis"]
    # a table of another tint: a numpy table raises in the binding, on the device the kernels refuse and touch nothing
    for tint in (0, 1):
        I = tr.intervals(4, tint)[1]
        with pytest.raises(ValueError):
            ctx.tec_search(vis4, tab, *args, tint, c["delays"], c["tecs"])
        with pytest.raises(ValueError):
            ctx.apply_tec(unit_sol(I, c["A"], 3), tab, vis4, c["a1"], c["a2"], tint)
        pk = to_dev(np.full((3, I, 12), 7.0))
        got, stats = ctx.tec_search(to_dev(vis4), to_dev(tab), to_dev(c["a1"]), to_dev(c["a2"]), c["A"], tint, c["delays"],
                                    c["tecs"], peaks=pk)
        assert list(host(stats)) == [0, 0, 0, 0, 0, 0, 0, 1] and (host(pk) == 7.0).all()
        out, wout = to_dev(np.full(vis4.shape, 5 + 1j)), to_dev(np.full(vis4.shape, 3.0))
        ctx.apply_tec(to_dev(unit_sol(I, c["A"], 3)), to_dev(tab), to_dev(vis4), to_dev(c["a1"]), to_dev(c["a2"]), tint, out=out,
                      weights_out=wout)
        assert (host(out) == 5 + 1j).all() and (host(wout) == 3.0).all()
    # cells outside the grid: a table of 4 delays x 3 TEC cells has the length of one of 3 x 4
    swapped = ((c["delays"][0], c["delays"][1], 3), (c["tecs"][0], c["tecs"][1], 4))
    invalid = tab.copy()
    invalid[0] = 0.0
    for t, axes in ((tab, swapped), (invalid, (c["delays"], c["tecs"]))):
        for form in (lambda x: x, to_dev):
            pk = form(np.full((3, 2, 12), 7.0))
            got, stats = ctx.tec_search(form(vis4), form(t), form(c["a1"]), form(c["a2"]), c["A"], 2, *axes, peaks=pk)
            assert list(np.asarray(host(stats) if form is to_dev else stats)) == [0, 0, 0, 0, 0, 0, 0, 1]
            assert (np.asarray(host(pk) if form is to_dev else pk) == 7.0).all()


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def fit_close(got, want, delays, tecs):
    sol, peaks, info, stats = got
    wsol, wpeaks, winfo, wstats = want
    assert np.array_equal(peaks[..., [0, 1, 8, 10]], wpeaks[..., [0, 1, 8, 10]]) and np.array_equal(info, winfo)
    assert np.abs(sol[..., 0] - wsol[..., 0]).max() <= TOL * delays[1] and np.abs(sol[..., 1] - wsol[..., 1]).max() <= TOL * tecs[1]
    assert np.abs(sol[..., 2:] - wsol[..., 2:]).max() <= TOL
    assert np.abs(peaks[..., 3] - wpeaks[..., 3]).max() <= TOL * delays[1]
    assert np.abs(peaks[..., 4] - wpeaks[..., 4]).max() <= TOL * tecs[1]
    assert np.abs(peaks[..., 5:8] - wpeaks[..., 5:8]).max() <= TOL
    assert np.array_equal(stats[[1, 2, 3, 4, 7]], wstats[[1, 2, 3, 4, 7]])


@pytest.mark.parametrize("flag_fraction,bounds", [(0.0, CLEAN_BOUNDS), (0.3, FLAGGED_BOUNDS)])
def test_tecfit_three_rounds(ctx, flag_fraction, bounds):
    c = tc.recovery_case(flag_fraction)
    A, T = c["A"], c["T"]
    tab = ctx.tec_tables(c["freq"], T, 0, c["delays"], c["tecs"])
    kw = dict(rounds=3, window=(2, 2), refant=0, niter=50)
    want = tr.tecfit(tab, c["vis"], c["a1"], c["a2"], A, wt=c["wt"], rounds=3, window_cells=(2, 2), refant=0, niter=50)
    got = ctx.tecfit(c["vis"], tab, c["a1"], c["a2"], A, 0, c["delays"], c["tecs"], weights=c["wt"], **kw)
    fit_close(got, want, c["delays"], c["tecs"])
    dgot = ctx.tecfit(to_dev(c["vis"]), to_dev(tab), to_dev(c["a1"]), to_dev(c["a2"]), A, 0, c["delays"], c["tecs"],
                      weights=dev(c["wt"]), **kw)
    assert all(same(host(d), g) for d, g in zip(dgot, got)), "host and device forms: the same bits"
    err = tc.errors(got[0], c["sol"], c["delays"], c["tecs"])
    print("tecfit", flag_fraction, err)
    assert all(e < b for e, b in zip(err, bounds[1]))
    one = ctx.tecfit(c["vis"], tab, c["a1"], c["a2"], A, 0, c["delays"], c["tecs"], weights=c["wt"], rounds=1, refant=0)
    assert all(e < b for e, b in zip(tc.errors(one[0], c["sol"], c["delays"], c["tecs"]), bounds[0]))
    # a warm start continues where the cold fit stood
    warm = ctx.tecfit(c["vis"], tab, c["a1"], c["a2"], A, 0, c["delays"], c["tecs"], weights=c["wt"], sol=one[0].copy(), rounds=1,
                      refant=0)
    wwant = tr.tecfit(tab, c["vis"], c["a1"], c["a2"], A, wt=c["wt"], sol=one[0].copy(), rounds=1, refant=0)
    fit_close(warm, wwant, c["delays"], c["tecs"])


# ---- apply ------------------------------------------------------------------------------------------------------------------------
def test_apply_tec(ctx):
    c = search_case(9, 4, 4, seed=41, A=6, T=8, tint=3)
    a1, a2, vis, wt = c["a1"], c["a2"], c["vis"], c["wt"]
    tab = ctx.tec_tables(c["freq"], 8, 3, c["delays"], c["tecs"])
    sol = tc.as_sol(c["true"], c["freq"])
    bound = 4e-13 * np.abs(vis)  # two table-recipe phasors and three products (the fringe apply test's bound)
    for inverse in (True, False):
        want, wwant = tr.apply(tab, sol, a1, a2, vis, wt, inverse=inverse)
        out, wout = ctx.apply_tec(sol, tab, vis, a1, a2, 3, inverse=inverse, weights=wt)
        assert (np.abs(out - want) <= bound).all() and np.array_equal(wout, wt)
        dout, dwout = ctx.apply_tec(to_dev(sol), to_dev(tab), to_dev(vis), to_dev(a1), to_dev(a2), 3, inverse=inverse,
                                    weights=to_dev(wt))
        assert same(host(dout), out) and same(host(dwout), wout)
    fwd, _ = ctx.apply_tec(sol, tab, vis, a1, a2, 3, inverse=False)
    back, ones = ctx.apply_tec(sol, tab, fwd, a1, a2, 3, inverse=True)
    assert (np.abs(back - vis) <= bound).all() and (ones == 1.0).all()
    # a NaN row, an antenna out of range: the value is kept, the weight is +0.0
    bad, b1 = sol.copy(), a1.copy()
    bad[1, 2, 1] = np.nan
    b1[0] = 6
    out, wout = ctx.apply_tec(bad, tab, vis, b1, a2, 3, weights=wt)
    hit = np.zeros(vis.shape, dtype=bool)
    hit[(b1 == 2) | (a2 == 2), 3:6] = True
    hit[0] = True
    assert np.array_equal(out[hit], vis[hit]) and not wout[hit].any() and not np.signbit(wout[hit]).any()
    assert np.array_equal(wout[~hit], wt[~hit]) and (np.abs(out - tr.apply(tab, sol, a1, a2, vis)[0])[~hit] <= bound[~hit]).all()
    # in place
    want, _ = ctx.apply_tec(sol, tab, vis, a1, a2, 3, weights=wt)
    v, w = vis.copy(), wt.copy()
    ctx.apply_tec(sol, tab, v, a1, a2, 3, weights=w, out=v, weights_out=w)
    assert same(v, want) and same(w, wt)
    dv, dw = to_dev(vis), to_dev(wt)
    ctx.apply_tec(to_dev(sol), to_dev(tab), dv, to_dev(a1), to_dev(a2), 3, weights=dw, out=dv, weights_out=dw)
    assert same(host(dv), want) and same(host(dw), wt)


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def test_composition_restores_the_averages(ctx):
    import gridhip
    c = tc.composition_case()
    tab = ctx.tec_tables(c["freq"], c["T"], 0, c["delays"], c["tecs"])
    before = np.abs(c["vis"].mean(axis=(1, 2)))
    sol, _, info, stats = ctx.tecfit(c["vis"], tab, c["a1"], c["a2"], c["A"], 0, c["delays"], c["tecs"], rounds=COMPOSITION_ROUNDS)
    out, _ = ctx.apply_tec(sol, tab, c["vis"], c["a1"], c["a2"], 0)
    after = np.abs(out.mean(axis=(1, 2)) - 1.0)
    print("composition", before.max(), after.max())
    assert before.max() < 0.5 and after.max() < COMPOSITION_BOUND and stats[4] == 0 and stats[7] == 0
    clock = gridhip.tec_clock(sol, tab)  # the clock delays come back from the effective ones
    assert np.abs(clock - c["true"][0]).max() < 1e-3 * c["delays"][1] + tab[12] * 1e-3 * c["tecs"][1]


def test_a_captured_chain_replays_to_the_eager_result(ctx):
    import torch
    c = tc.recovery_case(0.3)
    A = c["A"]
    tab = ctx.tec_tables(c["freq"], c["T"], 0, c["delays"], c["tecs"])
    dv, dw, dt, d1, d2 = to_dev(c["vis"]), to_dev(c["wt"]), to_dev(tab), to_dev(c["a1"]), to_dev(c["a2"])
    out, wout = torch.empty_like(dv), torch.empty_like(dw)

    def chain():
        fit = ctx.tecfit(dv, dt, d1, d2, A, 0, c["delays"], c["tecs"], weights=dw, rounds=3, niter=50)
        return fit + ctx.apply_tec(fit[0], dt, dv, d1, d2, 0, weights=dw, out=out, weights_out=wout)

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
    B, T, F, A, Nd, Nm, I = 3, 4, 5, 3, 6, 4, 2
    nt = tr.table_doubles(F, Nd, Nm)
    full = lambda m, val, dt=torch.float64: torch.full((m,), val, dtype=dt, device="cuda:0")  # noqa: E731
    n = B * T * F
    t = dict(f=full(F, 1.0e8), tab=full(nt, 7.0), v=full(n, 3 + 4j, torch.complex128), m=full(n, 1 - 1j, torch.complex128),
             w=full(n, 1.0), a1=full(B, 0, torch.int64), a2=full(B, 1, torch.int64), sol=full(I * A * 4, 0.5),
             pk=full(B * I * 12, 5.0), info=full(I * A, 4.0), s=full(8, 6.0), o=full(n, 8 + 0j, torch.complex128), wo=full(n, 9.0))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    NAN, INF = np.nan, np.inf

    def tb(F=F, T=T, tint=2, f=p["f"], Nd=Nd, Nm=Nm, tab=p["tab"]):
        return lib.gridhip_tec_tables_dev(h, F, T, tint, f, -1.0, 0.5, Nd, -1.0, 0.5, Nm, tab)

    def se(B=B, T=T, F=F, A=A, I=I, tab=p["tab"], v=p["v"], m=p["m"], w=p["w"], a1=p["a1"], a2=p["a2"], sol=p["sol"], j0=0, j1=Nd,
           m0=0, m1=Nm, pk=p["pk"], s=p["s"]):
        return lib.gridhip_tec_search_dev(h, B, T, F, A, I, tab, v, m, w, a1, a2, sol, j0, j1, m0, m1, pk, s)

    def ff(I=I, Nd=Nd, Nm=Nm, tab=p["tab"], v=p["v"], rounds=2, wj=1, wm=1, warm=0, sol=p["sol"], pk=p["pk"], info=p["info"],
           s=p["s"], niter=5, ref=0, A=A, mc=0.0, mh=0.0, tol=0.0):
        return lib.gridhip_tecfit_dev(h, B, T, F, A, I, Nd, Nm, tab, v, p["m"], p["w"], p["a1"], p["a2"], rounds, wj, wm, mc, mh,
                                      ref, niter, tol, warm, sol, pk, info, s)

    def ap(F=F, A=A, I=I, tab=p["tab"], sol=p["sol"], a1=p["a1"], inverse=1, v=p["v"], w=p["w"], o=p["o"], wo=p["wo"]):
        return lib.gridhip_apply_tec_dev(h, B, T, F, A, I, tab, sol, a1, p["a2"], inverse, v, w, o, wo)

    bad = [tb(F=0), tb(F=1025), tb(T=0), tb(tint=-1), tb(tint=5), tb(Nd=0), tb(Nd=4097), tb(Nm=0), tb(Nm=1025), tb(f=None),
           tb(tab=None), tb(tab=p["f"]), tb(f=at("tab", 8 * (nt - 1))),
           se(B=0), se(T=0), se(F=0), se(F=1025), se(A=1), se(I=0), se(I=5), se(tab=None), se(v=None), se(a1=None), se(a2=None),
           se(pk=None), se(s=None), se(j0=-1), se(j0=2, j1=2), se(j1=4097), se(m0=-1), se(m0=3, m1=3), se(m1=1025),
           se(v=at("v", 8)), se(m=at("m", 8)), se(pk=p["v"]), se(pk=p["sol"]), se(s=p["w"]), se(s=at("pk", 0)), se(pk=at("tab", 0)),
           ff(I=0), ff(I=5), ff(Nd=0), ff(Nd=4097), ff(Nm=0), ff(Nm=1025), ff(rounds=0), ff(rounds=5), ff(wj=-1), ff(wj=4097),
           ff(wm=-1), ff(wm=1025), ff(warm=2), ff(tab=None), ff(v=None), ff(sol=None), ff(pk=None), ff(info=None), ff(s=None),
           ff(niter=-1), ff(niter=100001), ff(ref=3), ff(mc=-1.0), ff(mc=NAN), ff(mh=-0.5), ff(mh=INF), ff(tol=-1.0), ff(tol=NAN),
           ff(sol=p["pk"]), ff(pk=p["v"]), ff(info=at("sol", 0)),
           ap(F=0), ap(F=1025), ap(A=1), ap(I=0), ap(I=5), ap(tab=None), ap(sol=None), ap(a1=None), ap(v=None), ap(o=None),
           ap(inverse=2), ap(inverse=-1), ap(v=at("v", 8)), ap(o=at("o", 8)), ap(o=at("v", 16)), ap(wo=at("w", 8)),
           ap(o=p["m"], wo=p["m"]), ap(wo=p["sol"]), ap(o=at("tab", 0))]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), [i for i, rc in enumerate(bad) if rc != _lib.EINVAL]
    assert lib.gridhip_tec_tile(None) == _lib.EINVAL
    assert se(A=1025) == _lib.EUNSUPPORTED and ff(A=1025) == _lib.EUNSUPPORTED and ap(A=1025) == _lib.EUNSUPPORTED
    assert tb(T=(1 << 20) + 1) == _lib.EUNSUPPORTED
    for fn, args in ((lib.gridhip_tec_tables_dev, (F, T, 2, p["f"], -1.0, 0.5, Nd, -1.0, 0.5, Nm, p["tab"])),
                     (lib.gridhip_tec_search_dev, (B, T, F, A, I, p["tab"], p["v"], p["m"], p["w"], p["a1"], p["a2"], p["sol"], 0, Nd, 0,
                                                   Nm, p["pk"], p["s"])),
                     (lib.gridhip_apply_tec_dev, (B, T, F, A, I, p["tab"], p["sol"], p["a1"], p["a2"], 1, p["v"], p["w"], p["o"], p["wo"]))):
        assert fn(None, *args) == _lib.EINVAL
    torch.cuda.synchronize()
    for key, val in (("f", 1.0e8), ("tab", 7.0), ("v", 3 + 4j), ("m", 1 - 1j), ("w", 1.0), ("sol", 0.5), ("pk", 5.0), ("info", 4.0),
                     ("s", 6.0), ("o", 8 + 0j), ("wo", 9.0)):
        assert bool((t[key] == val).all()), key
    # a table that is not one (its head holds 7.0): stats[7] = 1 and the sentinels stay
    assert se() == 0 and bool((t["pk"] == 5.0).all()) and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    t["s"].fill_(6.0)
    assert ff() == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1]) and bool((t["pk"] == 5.0).all())
    assert ap() == 0 and bool((t["o"] == 8 + 0j).all()) and bool((t["wo"] == 9.0).all())
    # in place is no overlap
    assert tb() == 0 and ap(o=p["v"], wo=p["w"]) == 0
    torch.cuda.synchronize()
