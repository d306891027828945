"""Rotation-measure synthesis and RM-CLEAN on the device (gridhip_rm_tables, gridhip_rmsynth, gridhip_rmclean and their
_dev forms) against the numpy restatement tests/rm_ref.py.  The table is compared with long-double values inside the bounds
rm_ref.check_tables states; from the library's table on, cube, model, maps and stats are compared bit for bit
(np.array_equal, NaN where NaN is specified): rounded products, sums in a fixed order and comparisons leave no tolerance
to state.  The shapes are the smallest at the edges of the kernels: the synthesis tile of rm_tile() either side of each
edge, one axis at a time around (M, C, J) = (65, 5, 65); for the clean every count of registers per lane (J up to 64, 128,
256, 512), the first and the last lag of the RMSF, exact ties across lanes and registers, and M off the four lines of
sight of a work-group."""
import ctypes as C
import math

import numpy as np
import pytest

import rm_ref as R
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

f64, c128 = np.float64, np.complex128
FWHM = 2.0 * math.sqrt(3.0) / 0.06
DPHI = FWHM / 4.0


def lam2_of(Cn):
    return np.linspace(0.03, 0.09, Cn) if Cn > 1 else np.array([0.05])


def grid_of(J):
    return -(J - 1) / 2 * DPHI, DPHI, J


_tables = {}


def table(ctx, Cn, J, weighted=False):
    """the library's table of (C, J), made once by the host form and never changed"""
    key = (Cn, J, weighted)
    if key not in _tables:
        w = np.linspace(0.5, 1.5, Cn) if weighted else None
        tab = ctx.rm_tables(lam2_of(Cn), grid_of(J), weights=w, fwhm=FWHM)
        tab.setflags(write=False)
        _tables[key] = tab
    return _tables[key]


class option:
    def __init__(self, ctx, key, value):
        self.ctx, self.key, self.value = ctx, key, value

    def __enter__(self):
        self.ctx.set_option(self.key, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.key, 0)


@pytest.fixture(scope="module")
def tile():
    import gridhip
    return gridhip.rm_tile()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,J,weighted", [(1, 1, False), (3, 64, True), (48, 129, True), (5, 512, False)])
def test_tables(ctx, Cn, J, weighted):
    lam2, w = lam2_of(Cn), (np.linspace(0.5, 1.5, Cn) if weighted else None)
    phi0, dphi, _ = grid_of(J)
    tab = table(ctx, Cn, J, weighted)
    assert tab.shape == (R.table_doubles(Cn, J),) and tab[0] == 1.0
    R.check_tables(tab, lam2, w, phi0, dphi, J, FWHM)
    dev = host(ctx.rm_tables(to_dev(lam2), grid_of(J), weights=None if w is None else to_dev(w), fwhm=FWHM))
    assert same(dev, np.array(tab)), "the device form's bits"
    # the numpy recipe agrees to the rounding of its own sin and cos
    assert np.abs(tab - R.tables(lam2, w, phi0, dphi, J, FWHM)).max() <= 1e-13


@pytest.mark.parametrize("lam2,w", [([0.1, np.nan, 0.3], None), ([0.1, 0.2, 0.3], [1.0, -1.0, 1.0]), ([0.1, 0.2, 0.3], [0.0, 0.0, 0.0]),
                                    ([0.1, 0.2, 0.3], [1.0, np.inf, 1.0])])
def test_tables_judged_on_the_device(ctx, lam2, w):
    lam2, w = np.array(lam2), None if w is None else np.array(w)
    for tab in (ctx.rm_tables(lam2, (-3.0, 1.5, 4), weights=w, fwhm=2.0),
                host(ctx.rm_tables(to_dev(lam2), (-3.0, 1.5, 4), weights=None if w is None else to_dev(w), fwhm=2.0))):
        assert tab[0] == 0.0 and not np.any(tab[R.HEAD:] != 0.0)
        R.check_tables(tab, lam2, w, -3.0, 1.5, 4, 2.0)


# ---- synthesis ---------------------------------------------------------------------------------------------------------------
def synth_case(ctx, M, Cn, J, seed=0, forms=("dev",)):
    rng = np.random.default_rng(1000 * seed + 7 * M + 3 * Cn + J)
    tab = table(ctx, Cn, J, weighted=Cn > 1)
    Q, U = rng.normal(size=(Cn, M)), rng.normal(size=(Cn, M))
    want, wstats = R.synth(tab, Q, U)
    for form in forms:
        if form == "dev":
            cube, stats = (host(x) for x in ctx.rmsynth(to_dev(Q), to_dev(U), to_dev(np.array(tab))))
        else:
            cube, stats = ctx.rmsynth(Q, U, np.array(tab))
        assert same(cube, want), f"({M}, {Cn}, {J}) [{form}]: {np.argwhere(cube != want)[:4].tolist()}"
        assert same(stats, wstats)
    # independently of the restatement: the whole cube against E^T (Q + iU), within 1e-12 sum_c kw_c |P_c|
    _, E, _, _ = R.parts(tab, Cn, J)
    ref = E.T @ (Q + 1j * U)
    scale = (np.abs(E[:, :1]) * np.abs(Q + 1j * U)).sum(axis=0)  # (|E[c][j]| = kw_c for every j)
    assert np.all(np.abs(want - ref) <= 1e-12 * scale[None, :])


def test_synth_along_m(ctx, tile):
    for M in sorted({1, 63, 64, 65, tile[0] - 1, tile[0], tile[0] + 1, 2 * tile[0] + 1}):
        synth_case(ctx, M, 5, 65, forms=("dev", "host") if M == 65 else ("dev",))


def test_synth_along_j(ctx, tile):
    for J in sorted({1, 63, 64, 65, 129, 512, tile[1] - 1, tile[1], tile[1] + 1}):
        synth_case(ctx, 65, 5, J)


def test_synth_along_c(ctx, tile):
    for Cn in sorted({1, tile[2] - 1, tile[2], tile[2] + 1, 2 * tile[2] + 3}):
        synth_case(ctx, 65, Cn, 65, forms=("dev", "host") if Cn == 2 * tile[2] + 3 else ("dev",))


def test_synth_bad_lines_of_sight(ctx, tile):
    Cn, J, M = 2 * tile[2] + 3, 65, tile[0] + 9
    rng = np.random.default_rng(11)
    tab = np.array(table(ctx, Cn, J, True))
    Q, U = rng.normal(size=(Cn, M)), rng.normal(size=(Cn, M))
    clean, _ = (host(x) for x in ctx.rmsynth(to_dev(Q), to_dev(U), to_dev(tab)))
    Q2, U2 = Q.copy(), U.copy()
    Q2[tile[2] + 1, 3], U2[0, tile[0] + 2] = np.nan, np.inf  # (the second chunk of the first tile, the second tile)
    for cube, stats in ([host(x) for x in ctx.rmsynth(to_dev(Q2), to_dev(U2), to_dev(tab))], ctx.rmsynth(Q2, U2, tab)):
        badcols = [3, tile[0] + 2]
        good = [m for m in range(M) if m not in badcols]
        assert np.isnan(cube[:, badcols].real).all() and np.isnan(cube[:, badcols].imag).all()
        assert same(cube[:, good], clean[:, good]) and stats[0] == 2 and not stats[1:].any()
        assert same(cube, R.synth(tab, Q2, U2)[0])


def test_synth_anchor_a_thin_source_on_a_grid_depth(ctx):
    Cn, J = 48, 129
    phi0, dphi, _ = grid_of(J)
    tab = table(ctx, Cn, J, False)
    amp = 0.7 * np.exp(0.6j)
    P = amp * np.exp(2j * (phi0 + 97 * dphi) * lam2_of(Cn))
    q, u = np.ascontiguousarray(P.real.reshape(Cn, 1, 1)), np.ascontiguousarray(P.imag.reshape(Cn, 1, 1))
    cube, stats = ctx.rmsynth(q, u, np.array(tab))
    assert cube.shape == (J, 1, 1) and np.argmax(np.abs(cube[:, 0, 0])) == 97 and abs(abs(cube[97, 0, 0]) - 0.7) <= 1e-12


# ---- RM-CLEAN ----------------------------------------------------------------------------------------------------------------
def clean_dev(ctx, tab, cube, model=None, **kw):
    dm = None if model is None else to_dev(model)
    if isinstance(kw.get("noise"), np.ndarray):
        kw["noise"] = to_dev(kw["noise"])
    return tuple(host(x) for x in ctx.rmclean(to_dev(cube), to_dev(np.array(tab)), model=dm, **kw))


def same_clean(what, got, want):
    model, cube, maps, stats = got
    wmodel, wcube, wmaps, wstats = want[:4]
    print(f"{what}: stats {stats}")
    assert same(stats, wstats), f"{what}: stats {stats} != {wstats}"
    assert same(maps, wmaps), f"{what}: maps differ at {np.argwhere(~((maps == wmaps) | (np.isnan(maps) & np.isnan(wmaps))))[:6].tolist()}"
    assert same(cube, wcube), f"{what}: cube"
    assert same(model, wmodel), f"{what}: model"


def generated(ctx, Cn, J, M, niter, restore=False, noise=0.02, **kw):
    """a generated case whose restatement never chose between two p closer than 1e-9 (the next seed otherwise)"""
    phi0, dphi, _ = grid_of(J)
    tab = table(ctx, Cn, J, False)
    for seed in range(20):
        rng = np.random.default_rng(100 * J + niter + 7919 * seed)
        Q, U, _ = R.sky(rng, lam2_of(Cn), phi0, dphi, J, M, noise=noise, edge=True)
        cube, _ = R.synth(tab, Q, U)
        want = R.rmclean(tab, cube, niter=niter, restore=restore, **kw)
        if want[4] >= 1e-9:
            return tab, cube, want
    raise AssertionError("no seed without a near tie")


@pytest.mark.parametrize("J", [1, 2, 64, 65, 129, 512])
@pytest.mark.parametrize("niter", [0, 1, 200])
def test_clean(ctx, J, niter):
    Cn = 48 if J > 1 else 3
    tab, cube, want = generated(ctx, Cn, J, 7, niter, gain=0.1, threshold=0.1)
    same_clean(f"J = {J}, niter = {niter}", clean_dev(ctx, tab, cube, gain=0.1, threshold=0.1, niter=niter), want)
    with option(ctx, "rm_stage", 1):
        same_clean(f"J = {J}, niter = {niter}, staged", clean_dev(ctx, tab, cube, gain=0.1, threshold=0.1, niter=niter), want)
    if niter == 200 and J > 2:
        assert want[3][1] > want[2].shape[1] and want[3][3] >= 1  # (components were taken, and the level was reached)


def test_clean_exact_ties_go_to_the_lowest_depth(ctx):
    J = 129
    tab = table(ctx, 48, J, False)
    pairs = [(10, 11), (5, 69), (3, 70)]  # neighbouring lanes; one lane, two registers; two lanes, two registers
    cube = np.full((J, len(pairs) + 1), 0.125 + 0.0625j, dtype=c128)
    for m, (a, b) in enumerate(pairs):
        cube[a, m], cube[b, m] = 3.0 - 4.0j, -4.0 + 3.0j  # |.|^2 = 25 both, exactly
    cube[:, 3] = 1.0 - 1.0j  # every depth ties: depth 0
    for stage in (0, 1):
        with option(ctx, "rm_stage", stage):
            got = clean_dev(ctx, tab, cube, gain=0.5, niter=1, threshold=0.01)
        same_clean(f"ties, stage {stage}", got, R.rmclean(tab, cube, gain=0.5, niter=1, threshold=0.01))
        model = got[0]
        for m, (a, b) in enumerate(pairs):
            assert model[a, m] == 0.5 * (3.0 - 4.0j) and np.count_nonzero(model[:, m]) == 1
        assert model[0, 3] == 0.5 - 0.5j and np.count_nonzero(model[:, 3]) == 1


def test_clean_a_nan_among_good_lines_of_sight(ctx):
    tab, cube, _ = generated(ctx, 48, 65, 6, 50, gain=0.1, threshold=0.1)
    cube = cube.copy()
    cube[40, 2] = np.nan + 0j
    cube[0, 5] = 1.0 + np.inf * 1j
    model = np.full(cube.shape, 0.25 - 0.5j)
    want = R.rmclean(tab, cube, model=model, gain=0.1, threshold=0.1, niter=50, restore=True)
    for stage in (0, 1):
        with option(ctx, "rm_stage", stage):
            got = clean_dev(ctx, tab, cube, model=model, gain=0.1, threshold=0.1, niter=50, restore=True)
        same_clean(f"NaN LOS, stage {stage}", got, want)
        assert got[3][0] == 2 and np.array_equal(got[2][:3, 2], [0, 3, -1]) and np.isnan(got[2][3:, [2, 5]]).all()
        assert same(got[1][:, [2, 5]], cube[:, [2, 5]]) and same(got[0][:, [2, 5]], model[:, [2, 5]])  # left untouched


def test_clean_stop_levels(ctx):
    tab, cube, _ = generated(ctx, 48, 65, 5, 300, gain=0.1, threshold=0.1)
    # by the threshold; by nsigma * sigma from a device element (the larger of the two); with a factor of 0
    for kw in (dict(threshold=0.2), dict(threshold=0.05, nsigma=3.0, noise=np.array([0.1])), dict(threshold=0.5, nsigma=3.0, noise=np.array([0.1])),
               dict(threshold=0.0, nsigma=5.0, noise=np.array([0.04]))):
        want = R.rmclean(tab, cube, gain=0.2, niter=300, **kw)
        got = clean_dev(ctx, tab, cube, gain=0.2, niter=300, **dict(kw))
        same_clean(str(kw), got, want)
        assert got[3][5] == max(kw["threshold"], kw.get("nsigma", 0.0) * float(kw.get("noise", [0.0])[0])) and got[3][3] == 5
        assert np.all(got[2][3] <= got[3][5] ** 2)
    got = ctx.rmclean(cube.copy(), np.array(tab), gain=0.2, niter=300, threshold=0.05, nsigma=3.0, noise=0.1)  # the host form, a number
    same_clean("host, noise a number", got, R.rmclean(tab, cube, gain=0.2, niter=300, threshold=0.05, nsigma=3.0, noise=[0.1]))
    # a NaN sigma: stats[6] = 1 and nothing else is touched, in both forms
    import torch
    dc, dm = to_dev(cube), torch.full(cube.shape, 2 - 1j, dtype=torch.complex128, device="cuda:0")
    model, res, maps, stats = ctx.rmclean(dc, to_dev(np.array(tab)), nsigma=2.0, noise=to_dev(np.array([np.nan])), model=dm)
    assert np.array_equal(host(stats), [0, 0, 0, 0, 0, 0, 1, 0]) and same(host(res), cube) and bool((dm == 2 - 1j).all())
    hc, hm = cube.copy(), np.full(cube.shape, 2 - 1j)
    model, res, maps, stats = ctx.rmclean(hc, np.array(tab), nsigma=2.0, noise=float("nan"), model=hm, restore=True)
    assert np.array_equal(stats, [0, 0, 0, 0, 0, 0, 1, 0]) and same(hc, cube) and np.all(hm == 2 - 1j)


def test_restore_and_a_model_carried_over(ctx):
    tab, cube, first = generated(ctx, 48, 129, 6, 5, gain=0.2, threshold=0.1)
    got1 = clean_dev(ctx, tab, cube, gain=0.2, threshold=0.1, niter=5)
    same_clean("first call", got1, first)
    for restore in (False, True):
        want = R.rmclean(tab, first[1], model=first[0], gain=0.2, threshold=0.1, niter=100, restore=restore)
        for stage in (0, 1):
            with option(ctx, "rm_stage", stage):
                got = clean_dev(ctx, tab, got1[1], model=got1[0], gain=0.2, threshold=0.1, niter=100, restore=restore)
            same_clean(f"second call, restore {restore}, stage {stage}", got, want)
    assert np.count_nonzero(first[0]) > 0 and want[3][1] > 0


def test_a_single_component_cleaned_and_restored_has_its_amplitude(ctx):
    Cn, J, L = 48, 129, 0.01
    phi0, dphi, _ = grid_of(J)
    tab = np.array(table(ctx, Cn, J, False))
    amps = np.array([1.0 * np.exp(0.3j), 0.4 * np.exp(2.0j), 2.5 * np.exp(-1.0j)])
    depths = [0, 64, 128]
    P = np.stack([a * np.exp(2j * (phi0 + j * dphi) * lam2_of(Cn)) for a, j in zip(amps, depths)], axis=1)
    cube, _ = ctx.rmsynth(np.ascontiguousarray(P.real), np.ascontiguousarray(P.imag), tab)
    model, rest, maps, stats = ctx.rmclean(cube, tab, gain=0.1, threshold=L, niter=2000, restore=True)
    assert stats[3] == 3 and np.array_equal(maps[2], depths)
    assert np.all(np.abs(np.sqrt(maps[3]) - np.abs(amps)) <= L), np.sqrt(maps[3])
    assert np.all(np.abs(maps[4] - (phi0 + np.array(depths) * dphi)) <= dphi)


# ---- the forms -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(ctx):
    """Q, U of 13 x 9 lines of sight, the table, and the restatement of rmsynth -> rmclean"""
    Cn, J = 35, 129
    phi0, dphi, _ = grid_of(J)
    tab = np.array(table(ctx, Cn, J, True))
    for seed in range(20):
        Q, U, _ = R.sky(np.random.default_rng(seed), lam2_of(Cn), phi0, dphi, J, 13 * 9, noise=0.02)
        cube, _ = R.synth(tab, Q, U)
        want = R.rmclean(tab, cube, gain=0.1, nsigma=5.0, noise=[0.02], niter=200, restore=True)
        if want[4] >= 1e-9:
            return tab, Q.reshape(Cn, 13, 9), U.reshape(Cn, 13, 9), cube, want
    raise AssertionError("no seed without a near tie")


def shaped(want):
    return tuple(x.reshape(x.shape[0], 13, 9) for x in want[:3]) + (want[3],)


def test_host_and_device_forms_and_two_runs(ctx, chain):
    import torch
    tab, Q, U, cube, want = chain
    kw = dict(gain=0.1, nsigma=5.0, niter=200, restore=True)
    hc, hs = ctx.rmsynth(Q, U, tab)
    assert same(hc, cube.reshape(hc.shape)) and hc.shape == (129, 13, 9)
    same_clean("host", ctx.rmclean(hc, tab, noise=np.array([0.02]), **kw), shaped(want))
    dq, du, dt, dn = to_dev(Q), to_dev(U), to_dev(tab), to_dev(np.array([0.02]))
    for run in range(2):
        dc, _ = ctx.rmsynth(dq, du, dt)
        assert same(host(dc), cube.reshape(hc.shape))
        same_clean(f"device, run {run}", tuple(host(x) for x in ctx.rmclean(dc, dt, noise=dn, **kw)), shaped(want))
    # a repeated call takes no memory
    out = torch.empty_like(dc)
    del dc
    ctx.rmclean(ctx.rmsynth(dq, du, dt, out=out)[0], dt, noise=dn, **kw)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    res = ctx.rmclean(ctx.rmsynth(dq, du, dt, out=out)[0], dt, noise=dn, **kw)
    torch.cuda.synchronize()
    assert res[1] is out and torch.cuda.mem_get_info()[0] == free
    same_clean("third run", tuple(host(x) for x in res), shaped(want))


def test_a_captured_chain_replays_to_the_eager_result(ctx, chain):
    import torch
    tab, Q, U, cube, want = chain
    kw = dict(gain=0.1, nsigma=5.0, niter=200, restore=True)
    dq, du, dt, dn = to_dev(Q), to_dev(U), to_dev(tab), to_dev(np.array([0.02]))
    out = torch.empty((129, 13, 9), dtype=torch.complex128, device="cuda:0")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds the counters
        ctx.rmclean(ctx.rmsynth(dq, du, dt, out=out)[0], dt, noise=dn, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        res = ctx.rmclean(ctx.rmsynth(dq, du, dt, out=out)[0], dt, noise=dn, **kw)  # (model None: zeroed inside the graph)
    torch.cuda.synchronize()
    for _ in range(2):
        for x in res[1:]:
            x.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        same_clean("replay", [host(x) for x in res], shaped(want))
    assert want[3][1] > 117 and want[3][3] > 0


# ---- the rules -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header through the C ABI on device memory, and the arrays as they were given."""
    import torch
    from gridhip import _lib
    lib, h = _lib.load(), ctx._h
    Cn, J, M = 2, 3, 4
    nt = R.table_doubles(Cn, J)
    full = lambda m, val, dt=torch.float64: torch.full((m,), val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(l=full(Cn, 0.5), w=full(Cn, 1.0), t=full(nt, 7.0), q=full(Cn * M, 1.0), u=full(Cn * M, 2.0),
             c=full(J * M, 3 + 4j, torch.complex128), m=full(J * M, 1 - 1j, torch.complex128), mp=full(7 * M, 5.0), s=full(8, 6.0),
             n=full(1, 0.5))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    NAN, INF = np.nan, np.inf

    def tb(C_=Cn, J=J, l=p["l"], w=p["w"], phi0=-1.0, dphi=1.0, fwhm=2.0, tab=p["t"]):
        return lib.gridhip_rm_tables_dev(h, C_, J, l, w, phi0, dphi, fwhm, tab)

    def sy(M=M, C_=Cn, J=J, tab=p["t"], q=p["q"], u=p["u"], c=p["c"], s=p["s"]):
        return lib.gridhip_rmsynth_dev(h, M, C_, J, tab, q, u, c, s)

    def cl(M=M, J=J, tab=p["t"], c=p["c"], m=p["m"], gain=0.1, thr=0.0, niter=5, nsigma=0.0, n=None, restore=0, mp=p["mp"], s=p["s"]):
        return lib.gridhip_rmclean_dev(h, M, J, tab, c, m, gain, thr, niter, nsigma, n, restore, mp, s)

    bad = [tb(C_=0), tb(C_=1025), tb(J=0), tb(J=513), tb(phi0=NAN), tb(phi0=INF), tb(dphi=0.0), tb(dphi=-1.0), tb(dphi=NAN),
           tb(dphi=INF), tb(fwhm=0.0), tb(fwhm=-2.0), tb(fwhm=NAN), tb(fwhm=INF), tb(l=None), tb(tab=None), tb(tab=p["l"]),
           tb(tab=at("w", -8 * (nt - 1))), tb(w=p["l"]), tb(l=at("t", 8 * (nt - 1))),
           sy(M=0), sy(C_=0), sy(C_=1025), sy(J=0), sy(J=513), sy(tab=None), sy(q=None), sy(u=None), sy(c=None), sy(s=None),
           sy(c=at("c", 8)), sy(c=p["q"]), sy(c=at("t", 0)), sy(s=p["u"]), sy(s=at("c", 16 * J * M - 8)), sy(u=p["q"]),
           sy(q=at("t", 8 * (nt - 1))),
           cl(M=0), cl(J=0), cl(J=513), cl(tab=None), cl(c=None), cl(mp=None), cl(s=None), cl(gain=NAN), cl(gain=INF), cl(thr=NAN),
           cl(thr=-INF), cl(niter=-1), cl(nsigma=-1.0), cl(nsigma=NAN), cl(nsigma=INF), cl(nsigma=2.0), cl(restore=2),
           cl(restore=-1), cl(restore=1, m=None), cl(c=at("c", 8)), cl(m=at("m", 8)), cl(m=p["c"]), cl(mp=p["c"]), cl(mp=p["m"]),
           cl(s=at("mp", 56 * M - 8)), cl(s=p["c"]), cl(c=p["t"]), cl(nsigma=1.0, n=at("c", 0)), cl(nsigma=1.0, n=p["s"])]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), [i for i, rc in enumerate(bad) if rc != _lib.EINVAL]
    for fn, args in ((lib.gridhip_rm_tables_dev, (Cn, J, p["l"], p["w"], -1.0, 1.0, 2.0, p["t"])),
                     (lib.gridhip_rmsynth_dev, (M, Cn, J, p["t"], p["q"], p["u"], p["c"], p["s"])),
                     (lib.gridhip_rmclean_dev, (M, J, p["t"], p["c"], p["m"], 0.1, 0.0, 5, 0.0, None, 0, p["mp"], p["s"]))):
        assert fn(None, *args) == _lib.EINVAL
    torch.cuda.synchronize()
    for key, val in (("l", 0.5), ("w", 1.0), ("t", 7.0), ("q", 1.0), ("u", 2.0), ("c", 3 + 4j), ("m", 1 - 1j), ("mp", 5.0),
                     ("s", 6.0), ("n", 0.5)):
        assert bool((t[key] == val).all()), key
    # a table that is not one (its head holds 7.0): stats[7] = 1 and the sentinels stay; then a valid one of another C or J
    assert sy() == 0 and bool((t["c"] == 3 + 4j).all()) and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    assert cl() == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    assert cl(nsigma=1.0, n=p["n"], restore=1) == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    assert bool((t["c"] == 3 + 4j).all()) and bool((t["m"] == 1 - 1j).all()) and bool((t["mp"] == 5.0).all())
    assert tb() == 0
    big = full(R.table_doubles(Cn, J + 1), 0.0)
    assert lib.gridhip_rm_tables_dev(h, Cn, J + 1, p["l"], None, -1.0, 1.0, 2.0, C.c_void_p(big.data_ptr())) == 0
    bigp = C.c_void_p(big.data_ptr())
    assert sy(tab=bigp) == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])       # the table's J is 4
    assert cl(tab=bigp) == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])
    assert sy(C_=1, q=p["q"], u=p["u"]) == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1])  # the table's C is 2
    assert bool((t["c"] == 3 + 4j).all()) and bool((t["m"] == 1 - 1j).all()) and bool((t["mp"] == 5.0).all())
    # device-judged: lam2 all equal is fine (a = 0), a NaN is not; and the host forms leave their arrays alone too
    t["l"][1] = float("nan")
    assert tb() == 0 and sy() == 0 and np.array_equal(host(t["s"]), [0, 0, 0, 0, 0, 0, 0, 1]) and bool((t["c"] == 3 + 4j).all())
    invalid = host(t["t"])
    hq, hu, hc, hm = np.ones((Cn, M)), np.ones((Cn, M)), np.full((J, M), 3 + 4j), np.full((J, M), 1 - 1j)
    cube, stats = ctx.rmsynth(hq, hu, invalid, out=hc)
    assert cube is hc and np.all(hc == 3 + 4j) and np.array_equal(stats, [0, 0, 0, 0, 0, 0, 0, 1])
    model, cube, maps, stats = ctx.rmclean(hc, invalid, model=hm, restore=True)
    assert np.all(hc == 3 + 4j) and np.all(hm == 1 - 1j) and np.array_equal(stats, [0, 0, 0, 0, 0, 0, 0, 1])
    # and the valid corners next to the refusals: no weights, no model, an output that ends where an input begins
    t["l"][1] = 0.25
    assert tb(w=None) == 0 and sy() == 0 and cl(m=None) == 0 and cl(nsigma=1.0, n=p["n"], restore=1) == 0
    ctx.synchronize()
    assert host(t["s"])[7] == 0 and host(t["s"])[6] == 0
