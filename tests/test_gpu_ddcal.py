"""Direction-dependent calibration on the device (gridhip_ddcal*, gridhip_dd_subtract*, gridhip_imager_peel_dev) against
the numpy restatement tests/ddcal_ref.py, at fixed niter and tol = 0 so that rounding cannot move the stop.

Tolerances are those of test_gpu_gaincal.py, because the sums meet the same way (fp64 atomics, at most a few thousand
terms per antenna): gains 1e-10 of the largest |g|; the integer entries of stats exact; chi^2 and chi^2 at g = 1 1e-9
relative; the last rel 1e-9 + 1e-9 rel; the subtraction 1e-12 of the largest |vis_in|.

Precondition.  The LDL^H divides by its pivots, so the 1e-10 holds for a well-conditioned H only, and whether a cell is
solved must not depend on rounding: every solve case first asserts that every pivot ratio d_j / H[j,j] the reference saw
is above 1e-6 - or, in the cases meant to have unsolved cells, above 1e-6, exactly 0 or below 1e-14."""
import ctypes as C

import numpy as np
import pytest

import ddcal_ref as R
from test_ddcal_host import dd_case
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-10
CHUNK = 4096  # the iteration kernel's chunk (GC_CHUNK, csrc/imaging.h)
c128, f64, i64 = np.complex128, np.float64, np.int64


def dev(x):
    return None if x is None else to_dev(x)


def solve(ctx, V, M, a1, a2, A, slot=None, T=1, wt=None, mode=0, refant=0, niter=4, tol=0.0, gains=None, form="dev"):
    """-> (gains, stats) as numpy arrays, by the device form (torch tensors) or the host form (numpy arrays)"""
    kw = dict(nslots=T, phase_only=bool(mode), refant=None if refant < 0 else refant, niter=niter, tol=tol)
    a1, a2 = np.asarray(a1, dtype=i64), np.asarray(a2, dtype=i64)
    slot = None if slot is None else np.asarray(slot, dtype=i64)
    V, M = np.asarray(V, dtype=c128), np.ascontiguousarray(M, dtype=c128)
    wt = None if wt is None else np.asarray(wt, dtype=f64)
    if form == "host":
        return ctx.ddcal(V, M, a1, a2, A, slot=slot, weights=wt, gains=None if gains is None else gains.copy(), **kw)
    g, st = ctx.ddcal(dev(V), dev(M), dev(a1), dev(a2), A, slot=dev(slot), weights=dev(wt),
                      gains=None if gains is None else dev(gains), **kw)
    return host(g), host(st)


def agree(what, g, st, gr, sr):
    gmax = np.abs(gr).max()
    eg = np.abs(g - gr).max() / gmax
    print(f"{what}: gains {eg:.2e}  rel {st[1]:.3e} / {sr[1]:.3e}  chi2 {st[2]:.6e} / {sr[2]:.6e}  chi2_0 {st[3]:.6e} / "
          f"{sr[3]:.6e}  ints {st[[0, 4, 5, 6, 7]]}")
    assert g.shape == gr.shape and eg <= TOL, what
    assert np.array_equal(st[[0, 4, 5, 6, 7]], sr[[0, 4, 5, 6, 7]]), what
    assert abs(st[3] - sr[3]) <= 1e-9 * sr[3] and abs(st[2] - sr[2]) <= 1e-9 * sr[2], what
    if np.isnan(sr[1]):
        assert np.isnan(st[1]), what
    else:
        assert abs(st[1] - sr[1]) <= 1e-9 + 1e-9 * sr[1], what


def reference(what, V, M, a1, a2, A, unsolved=False, **kw):
    """the restatement's result, after the precondition on the pivots"""
    piv = []
    gr, sr, worst = R.ddcal(V, M, a1, a2, A, pivots=piv, **{"niter": 4, "tol": 0.0, **kw})
    piv = np.array(piv)
    print(f"{what}: smallest pivot ratio {worst:.3e} of {len(piv)}")
    if unsolved:
        assert np.all((piv > 1e-6) | (piv == 0.0) | (piv < 1e-14)), what
    else:
        assert np.all(piv > 1e-6), what
    return gr, sr


def both(ctx, what, V, M, a1, a2, A, forms=("dev", "host"), unsolved=False, **kw):
    gr, sr = reference(what, V, M, a1, a2, A, unsolved=unsolved, **kw)
    out = None
    for form in forms:
        g, st = solve(ctx, V, M, a1, a2, A, form=form, **kw)
        agree(f"{what} [{form}]", g, st, gr, sr)
        out = g, st
    return out, (gr, sr)


def stream(rng, n, A, T, D, order="time", near=0):
    """n visibilities on random baselines (near > 0: antenna a only with a + 1 .. a + near, a sparse set that keeps n
    small at many antennas), D point-source models, corrupted by D gain sets and a little noise"""
    a1 = rng.integers(0, A, n)
    a2 = (a1 + rng.integers(1, near + 1 if near else A, n)) % A
    sl = rng.integers(0, T, n)
    if order == "time":
        sl = np.sort(sl)
    u, v = rng.uniform(-300, 300, n), rng.uniform(-300, 300, n)
    l, m = rng.uniform(-0.05, 0.05, D), rng.uniform(-0.05, 0.05, D)
    M = np.exp(-2j * np.pi * (u[None] * l[:, None] + v[None] * m[:, None])) * rng.uniform(1, 3, D)[:, None]
    gt = (1 + 0.2 * rng.normal(size=(D, T, A))) * np.exp(1j * rng.uniform(-1, 1, (D, T, A)))
    V = R.model_sum(gt, a1, a2, sl, M) + 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return a1, a2, sl, V, M, rng.uniform(0.5, 2, n)


# ---- one direction is gaincal ------------------------------------------------------------------------------------------------
def test_one_direction_agrees_with_gaincal_on_the_device(ctx):
    a1, a2, sl, V, M, w, _ = dd_case(np.random.default_rng(31), 7, 3, 1, noise=0.05, weights=True)
    for mode in (0, 1):
        g, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, mode=mode, niter=9, refant=3)
        g0, st0 = ctx.gaincal(dev(V), dev(M[0]), dev(a1), dev(a2), 7, slot=dev(sl), nslots=3, weights=dev(w),
                              phase_only=bool(mode), refant=3, niter=9, tol=0.0)
        g0, st0 = host(g0), host(st0)
        print(f"mode {mode}: {np.abs(g[0] - g0).max() / np.abs(g0).max():.2e}")
        assert g.shape == (1, 3, 7) and np.abs(g[0] - g0).max() <= TOL * np.abs(g0).max()
        assert np.array_equal(st[[0, 4, 5, 6, 7]], st0[[0, 4, 5, 6, 7]]) and np.allclose(st[1:4], st0[1:4], rtol=1e-9)


# ---- every baseline, every D ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_baseline_three_intervals(ctx, D, mode):
    A = 7 if D < 5 else 12  # (11 baselines per interval and antenna: at least D, so the normal matrix has full rank)
    a1, a2, sl, V, M, w, _ = dd_case(np.random.default_rng(40 + D), A, 3, D, noise=0.05, weights=True)
    both(ctx, f"A={A} T=3 D={D} mode={mode}", V, M, a1, a2, A, slot=sl, T=3, wt=w, mode=mode, niter=9, refant=3)


def test_no_visibilities_and_no_iterations(ctx):
    e = np.zeros(0)
    (g, st), _ = both(ctx, "n=0", e.astype(c128), np.zeros((2, 0), dtype=c128), e.astype(i64), e.astype(i64), 3, niter=3,
                      unsolved=True)
    assert g.shape == (2, 1, 3) and np.all(g == 1) and st[7] == 3 and st[0] == 3 and st[1] == 0
    a1, a2, sl, V, M, w, _ = dd_case(np.random.default_rng(32), 4, 2, 2, weights=True)
    (g, st), _ = both(ctx, "niter=0", V, M, a1, a2, 4, slot=sl, T=2, wt=w, niter=0)
    assert np.all(g == 1) and st[0] == 0 and st[7] == 8 and st[4] == len(V)
    warm = (np.arange(16).reshape(2, 2, 4) - 2.5j + 1).astype(c128)
    (g, st), _ = both(ctx, "niter=0 warm", V, M, a1, a2, 4, slot=sl, T=2, wt=w, niter=0, gains=warm)
    assert np.array_equal(g, warm)
    both(ctx, "n=1", [2 + 1j], [[1 - 1j], [0.5 + 2j]], [0], [1], 2, unsolved=True)


# ---- degenerate data -----------------------------------------------------------------------------------------------------------
def test_missing_antennas_intervals_refant_autos_and_indices_out_of_range(ctx):
    rng = np.random.default_rng(33)
    A, T, D = 6, 4, 2
    a1, a2, sl, V, M, w, _ = dd_case(rng, A, T, D, noise=0.05, weights=True)
    keep = (a1 != 4) & (a2 != 4) & (sl != 2) & ~((sl == 1) & ((a1 == 0) | (a2 == 0)))  # antenna 4, interval 2: no data;
    a1, a2, sl, V, w, M = *(x[keep] for x in (a1, a2, sl, V, w)), M[:, keep]           # refant 0 unsolved in interval 1
    warm = (1 + 0.2 * rng.normal(size=(D, T, A))) * np.exp(1j * rng.uniform(-1, 1, (D, T, A)))
    for gains in (None, warm):
        (g, st), _ = both(ctx, f"missing data warm={gains is not None}", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6,
                          gains=gains, unsolved=True)
        start = np.ones((D, T, A)) if gains is None else warm
        assert st[7] == T + A - 1 + 1  # antenna 4 everywhere, the rest of interval 2, refant 0 in interval 1
        assert np.array_equal(g[:, :, 4], start[:, :, 4]) and np.array_equal(g[:, 2], start[:, 2])
        assert np.array_equal(g[:, 1, 0], start[:, 1, 0])
        assert np.all(g[:, [0, 3], 0].imag == 0) and np.all(g[:, [0, 3], 0].real > 0)
    extra = np.array([[2, 2, 0], [5, 5, 3], [-1, 2, 0], [A, 2, 0], [1, -1, 0], [1, A, 3], [0, 1, -1], [0, 1, T]])
    n0, ne = len(a1), len(extra)
    a1x, a2x, slx = (np.concatenate([x, extra[:, i]]) for i, x in enumerate((a1, a2, sl)))
    Vx, wx = np.concatenate([V, np.full(ne, 5 + 5j)]), np.concatenate([w, np.ones(ne)])
    Mx = np.concatenate([M, np.full((D, ne), 1 - 2j)], axis=1)
    order = rng.permutation(n0 + ne)
    (g0, st0), _ = both(ctx, "without the dropped", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6, forms=("dev",), unsolved=True)
    (g1, st1), _ = both(ctx, "with the dropped", Vx[order], Mx[:, order], a1x[order], a2x[order], A, slot=slx[order], T=T,
                        wt=wx[order], niter=6, unsolved=True)
    assert st1[6] == ne and st0[6] == 0 and st1[4] == st0[4] == n0
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max()


def test_flagged_nan_and_inf_contribute_exactly_nothing(ctx):
    rng = np.random.default_rng(34)
    a1, a2, sl, V, M, w, _ = dd_case(rng, 5, 2, 3, noise=0.05, weights=True)
    n = len(a1)
    (g0, st0), _ = both(ctx, "clean", V, M, a1, a2, 5, slot=sl, T=2, wt=w, niter=6, forms=("dev",))
    bad = rng.choice(n, 12, replace=False)
    Vx, Mx, wx = np.tile(V, 2), np.tile(M, (1, 2)), np.concatenate([w, np.zeros(n)])  # every visibility again, flagged ...
    wx[n + bad[:4]], wx[n + bad[4:8]] = np.nan, -1.0
    Vx[n + bad[:6]] = [np.nan, np.inf, -np.inf, np.nan + 1j * np.inf, np.nan, np.inf]  # ... and carrying NaN and Inf in V
    for d in range(3):                                                                 # and in every model row
        Mx[d, n + bad[6 + 2 * d]], Mx[d, n + bad[7 + 2 * d]] = np.nan, np.inf
    order = rng.permutation(2 * n)
    (g1, st1), _ = both(ctx, "flagged", Vx[order], Mx[:, order], np.tile(a1, 2)[order], np.tile(a2, 2)[order], 5,
                        slot=np.tile(sl, 2)[order], T=2, wt=wx[order], niter=6)
    assert st1[5] == n and np.array_equal(st1[[0, 4, 6, 7]], st0[[0, 4, 6, 7]])
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max() and np.isfinite(st1).all()


def test_a_duplicate_direction_and_a_zero_direction_are_unsolved(ctx):
    rng = np.random.default_rng(35)
    a1, a2, sl, V, M, w, _ = dd_case(rng, 6, 2, 3, noise=0.05, weights=True)
    warm = (1 + 0.2 * rng.normal(size=(3, 2, 6))) * np.exp(1j * rng.uniform(-1, 1, (3, 2, 6)))
    dup, zero = M.copy(), M.copy()
    dup[2] = dup[0]
    warm_dup = warm.copy()
    warm_dup[2] = warm_dup[0]  # (equal models AND equal gains: the two regressors are the same bits, the pivot is exactly 0)
    zero[1] = 0
    for what, Mx, gains in (("duplicate", dup, warm_dup), ("zero", zero, warm)):
        (g, st), _ = both(ctx, what, V, Mx, a1, a2, 6, slot=sl, T=2, wt=w, niter=4, gains=gains, unsolved=True)
        assert st[7] == 12 and np.array_equal(g, gains) and st[1] == 0


# ---- chunking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_around_one_chunk(ctx, n):
    a1, a2, sl, V, M, w = stream(np.random.default_rng(n), n, 8, 3, 2)
    both(ctx, f"n={n}", V, M, a1, a2, 8, slot=sl, T=3, wt=w, niter=3, forms=("dev",))


def test_interval_change_on_a_chunk_boundary_and_inside_a_step(ctx):
    rng = np.random.default_rng(36)
    n = 3 * CHUNK
    a1, a2, _, V, M, w = stream(rng, n, 8, 1, 3)
    for what, sl in (("on the boundary", np.repeat([0, 1, 2], CHUNK)),
                     ("one before and one after", np.repeat([0, 1, 2], [CHUNK - 1, CHUNK + 2, CHUNK - 1])),
                     ("every visibility", np.arange(n) % 3)):
        both(ctx, f"interval change {what}", V, M, a1, a2, 8, slot=sl, T=3, wt=w, niter=3, forms=("dev",))


@pytest.mark.parametrize("D", [2, 4])  # (four visibilities of a lane at once, and one at a time)
def test_unordered_slots_agree_with_the_sorted_stream(ctx, D):
    rng = np.random.default_rng(37)
    n, A, T = 2 * CHUNK + 77, 16, 5
    a1, a2, sl, V, M, w = stream(rng, n, A, T, D)
    (g0, _), _ = both(ctx, "sorted", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=4, forms=("dev",))
    o = rng.permutation(n)
    (g1, _), _ = both(ctx, "permuted", V[o], M[:, o], a1[o], a2[o], A, slot=sl[o], T=T, wt=w[o], niter=4, forms=("dev",))
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max()


def test_ranges_of_several_chunks(ctx):
    """More chunks than the launch has work-groups: a work-group then takes a contiguous range of several chunks - the only
    size at which that path runs.  D = 3 at A = 500 takes 84 KB of LDS, so the launch has one work-group (of 1024
    threads) per CU and the path starts at the smallest n there is: one chunk more than CUs.  One iteration keeps the numpy
    reference at a few seconds."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = (ncu + 1) * CHUNK + 5
    a1, a2, sl, V, M, w = stream(np.random.default_rng(38), n, 500, 3, 3)
    both(ctx, f"n={n}", V, M, a1, a2, 500, slot=sl, T=3, wt=w, niter=1, forms=("dev",))


# ---- the LDS table's edges, the work-group sizes, and the limit on D * A * T -------------------------------------------------
def sparse(seed, A, D, T=2):
    """12 visibilities per antenna and interval on the baselines (a, a + 1 .. a + 6): n stays small at many antennas"""
    a1, a2, sl, V, M, w = stream(np.random.default_rng(seed), 12 * A * T, A, T, D, near=6)
    a1[:4], a2[:4] = [0, A - 1, A - 2, 0], [A - 1, 0, A - 1, 1]  # the table's last rows are used
    return a1, a2, sl, V, M, w


@pytest.mark.parametrize("D,over", [(1, 0), (1, 1), (3, 0), (3, 1), (8, 0), (8, 1)])
def test_lds_table_edges(ctx, D, over):
    import gridhip
    A = gridhip.ddcal_lds_antennas(D) + over  # the last size of the LDS path, the first of the global one
    a1, a2, sl, V, M, w = sparse(1000 * D + over, A, D)
    both(ctx, f"D={D} A={A}", V, M, a1, a2, A, slot=sl, T=2, wt=w, niter=2, forms=("dev",))


@pytest.mark.parametrize("A", [243, 244, 487, 488])
def test_work_group_sizes(ctx, A):
    """D = 3 takes 168 B of LDS per antenna: four tables (and 64 B each) fit in 160 KB up to A = 243 - work-groups of 256
    threads - two up to A = 487 - 512 threads - and one above - 1024 threads."""
    a1, a2, sl, V, M, w = sparse(A, A, 3)
    both(ctx, f"A={A}", V, M, a1, a2, A, slot=sl, T=2, wt=w, niter=2, forms=("dev",))


def test_table_limit(ctx):
    import torch
    from gridhip import GridHipError, _lib
    A, T, D = 512, 1024, 4  # D * A * T = 2^21, the stated limit
    rng = np.random.default_rng(39)
    a1, a2, sl, V, M, w = stream(rng, 2000, A, T, D)
    g = torch.full((D, T, A), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    g1, st = ctx.ddcal(dev(V), dev(M), dev(a1), dev(a2), A, slot=dev(sl), nslots=T, niter=2, tol=0.0, gains=g)
    st = host(st)
    assert st[0] == 2 and st[4] == 2000 and np.isfinite(st).all()  # (2000 visibilities cannot solve anything: all unsolved)
    assert st[7] == A * T and bool((g == 7 + 7j).all())
    g = torch.full((D, T, A + 1), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    with pytest.raises(GridHipError) as ei:
        ctx.ddcal(dev(V), dev(M), dev(a1), dev(a2), A + 1, slot=dev(sl), nslots=T, gains=g)
    assert ei.value.code == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((g == 7 + 7j).all())
    with pytest.raises(GridHipError) as ei:
        ctx.dd_subtract(g, dev(M), dev(a1), dev(a2), slot=dev(sl))
    assert ei.value.code == _lib.EUNSUPPORTED


# ---- the stop on the device ----------------------------------------------------------------------------------------------------
def test_stop_on_the_device(ctx):
    """The device's rel is within 1e-9 + 1e-9 rel of the reference's (asserted below), so a stop that the reference takes
    with rel <= 0.9 tol after rel >= 1.1 tol at tol = 1e-6 - margins of 1e-7, a hundred times that bound - cannot be
    moved by rounding.  (The iteration here gains a factor of about 3.5 per step: the seed was chosen so.)"""
    a1, a2, sl, V, M, w, _ = dd_case(np.random.default_rng(300), 7, 2, 2, noise=0.02, weights=True)
    tol, hist = 1e-6, []
    gr, sr, worst = R.ddcal(V, M, a1, a2, 7, slot=sl, T=2, wt=w, niter=150, tol=tol, history=hist)
    k = len(hist)
    assert k < 150 and hist[-1] <= 0.9 * tol and hist[-2] >= 1.1 * tol and sr[0] == k and worst > 1e-6
    g, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=2, wt=w, niter=150, tol=tol)
    agree("stopped", g, st, gr, sr)
    assert st[0] == k
    # exactly k iterations without a stop rule give the same gains: the 150 - k later launches changed nothing
    g2, st2 = solve(ctx, V, M, a1, a2, 7, slot=sl, T=2, wt=w, niter=k, tol=0.0)
    assert st2[0] == k and np.abs(g2 - g).max() <= TOL * np.abs(g).max() and abs(st2[1] - st[1]) <= 1e-9


def test_warm_start_reproduces_a_split_solve(ctx):
    a1, a2, sl, V, M, w, _ = dd_case(np.random.default_rng(41), 6, 2, 3, noise=0.05, weights=True)
    k = 4  # even: the second half then averages on the same iterations as the whole
    whole, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=2 * k, refant=-1)
    half, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1)
    rest, st = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1, gains=half)
    assert st[0] == k and np.abs(rest - whole).max() <= TOL * np.abs(whole).max()
    both(ctx, "warm", V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, gains=half)


# ---- subtract ------------------------------------------------------------------------------------------------------------------
def test_subtract_every_subset_in_place_no_input_and_rows_out_of_range(ctx):
    import itertools
    import torch
    rng = np.random.default_rng(42)
    n, A, T, D = CHUNK + 33, 6, 3, 3
    a1, a2, sl, V, M, _ = stream(rng, n, A, T, D)
    a1[:6], a2[:6], sl[:6] = [-1, A, 0, 0, 1, 1], [0, 1, -1, A, 2, 1], [0, 0, 0, 0, T, 0]  # out of range; an autocorrelation
    g = (1 + 0.3 * rng.normal(size=(D, T, A))) * np.exp(1j * rng.uniform(-2, 2, (D, T, A)))
    scale = np.abs(V).max()
    for k in range(D + 1):
        for dirs in itertools.combinations(range(D), k):
            want = R.dd_subtract(g, M, a1, a2, slot=sl, directions=dirs, vis=V)
            got = [ctx.dd_subtract(g, M, a1, a2, slot=sl, directions=dirs, vis=V),
                   host(ctx.dd_subtract(dev(g), dev(M), dev(a1), dev(a2), slot=dev(sl), directions=dirs, vis=dev(V)))]
            for o in got:
                assert np.abs(o - want).max() <= 1e-12 * scale, dirs
                assert np.array_equal(o[:5], V[:5])  # (row 5 is an autocorrelation in range: subtracted like any other)
            if k == 0:
                assert np.array_equal(got[0], V) and np.array_equal(got[1], V)
    # no input: the corrupted model itself; in place
    want = R.dd_subtract(g, M, a1, a2, slot=sl)
    for o in (ctx.dd_subtract(g, M, a1, a2, slot=sl), host(ctx.dd_subtract(dev(g), dev(M), dev(a1), dev(a2), slot=dev(sl)))):
        assert np.abs(o - want).max() <= 1e-12 * np.abs(want).max() and np.all(o[:5] == 0)
    dv = dev(V)
    out = ctx.dd_subtract(dev(g), dev(M), dev(a1), dev(a2), slot=dev(sl), directions=[0, 2], vis=dv, out=dv)
    assert out is dv
    torch.cuda.synchronize()
    assert np.abs(host(dv) - R.dd_subtract(g, M, a1, a2, slot=sl, directions=[0, 2], vis=V)).max() <= 1e-12 * scale
    # one direction corrected afterwards is apply_gains on its slice
    one = ctx.apply_gains(dev(g)[1], dev(V), dev(a1), dev(a2), slot=dev(sl))[0]
    assert one.shape == (n,)


@pytest.mark.parametrize("n", [0, 1, 257])  # none, one, one work-group and one
def test_subtract_host_and_device_forms_give_the_same_bits(ctx, n):
    """Every staging branch of gridhip_dd_subtract: slot and vis_in present and null, out of place and in place.  The
    subtraction is a fixed sequence of rounded operations per visibility, so the two forms give the same bits; the
    restatement holds within the 1e-12 of the largest visibility of the test above."""
    from test_gpu_gaincal import both_forms
    rng = np.random.default_rng(400 + n)
    A, T, D = 3, 2, 2
    a1, a2, sl, V, M, _ = stream(rng, n, A, T, D)
    M = np.ascontiguousarray(M)
    g = (1 + 0.3 * rng.normal(size=(D, T, A))) * np.exp(1j * rng.uniform(-2, 2, (D, T, A)))
    for slot in (sl, None):
        gg = g if slot is not None else np.ascontiguousarray(g[:, :1])
        for given in (True, False):
            for in_place in ((False, True) if given else (False,)):
                for dirs in ([0, 1], [1]):
                    vin = V.copy() if given else None
                    vout = vin if in_place else np.full(n, 7 - 7j)
                    bits = sum(1 << d for d in dirs)
                    hst, dvc = both_forms(ctx, "dd_subtract", [n, A, gg.shape[1], D, a1, a2, slot, gg, M, bits, vin, vout])
                    what = (n, slot is not None, given, in_place, dirs)
                    for k in hst:
                        assert hst[k].tobytes() == dvc[k].tobytes(), what
                    for x in (a1, a2, gg, M) + ((vin,) if given and not in_place else ()):
                        assert hst[id(x)].tobytes() == x.tobytes(), what  # inputs as they were
                    want = R.dd_subtract(gg, M, a1, a2, slot=slot, directions=dirs, vis=vin if given else None)
                    if n:
                        scale = np.abs(V).max() if given else np.abs(want).max()
                        assert np.abs(hst[id(vout)] - want).max() <= 1e-12 * scale, what


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header, through the C ABI on device memory: GRIDHIP_EINVAL and the outputs as they were given."""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    n, A, T, D = 5, 3, 2, 2
    full = lambda shape, val, dt=torch.complex128: torch.full(shape, val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(a1=to_dev(np.array([0, 0, 1, 0, 1], dtype=i64)), a2=to_dev(np.array([1, 2, 2, 1, 2], dtype=i64)),
             sl=to_dev(np.array([0, 0, 0, 1, 1], dtype=i64)), v=full((2 * n,), 2 + 1j), m=full((D * n,), 1 - 1j),
             w=full((n,), 1.5, torch.float64), g=full((D * T * A + 1,), 7 + 7j), st=full((8,), 9.0, torch.float64),
             o=full((n,), 3 + 3j))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    h = ctx._h

    def dd(n=n, A=A, T=T, D=D, a1=p["a1"], a2=p["a2"], sl=p["sl"], v=p["v"], m=p["m"], w=p["w"], mode=0, ref=0, warm=0,
           niter=3, tol=0.0, g=p["g"], st=p["st"]):
        return lib.gridhip_ddcal_dev(h, n, A, T, D, a1, a2, sl, v, m, w, mode, ref, warm, niter, tol, g, st)

    def sb(n=n, A=A, T=T, D=D, a1=p["a1"], a2=p["a2"], sl=p["sl"], g=p["g"], m=p["m"], dirs=3, v=p["v"], o=p["o"]):
        return lib.gridhip_dd_subtract_dev(h, n, A, T, D, a1, a2, sl, g, m, dirs, v, o)

    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    bad = [dd(n=-1), dd(A=1), dd(T=0), dd(D=0), dd(D=9), dd(D=-1), dd(sl=None), dd(a1=None), dd(a2=None), dd(v=None),
           dd(m=None), dd(g=None), dd(niter=-1), dd(tol=-1.0), dd(tol=float("nan")), dd(mode=2), dd(mode=-1), dd(ref=A),
           dd(g=p["v"]), dd(g=p["m"]), dd(g=p["w"]), dd(g=p["a1"]), dd(g=p["a2"]), dd(g=p["sl"]),
           dd(g=at("m", 16 * D * n - 8)),  # gains over the last row of model_vis only: the larger array is tested
           dd(m=at("g", 16 * (D * T * A - 1))),  # model_vis over the last gain of the last direction
           sb(n=-1), sb(A=1), sb(T=0), sb(D=0), sb(D=9), sb(sl=None), sb(a1=None), sb(a2=None), sb(g=None), sb(m=None),
           sb(o=None), sb(dirs=4), sb(dirs=7), sb(dirs=-1), sb(dirs=1 << 62), sb(o=p["g"]), sb(o=at("g", 16 * (D * T * A - 1))),
           sb(o=p["m"]), sb(o=at("m", 16 * (D * n - 1))), sb(o=p["a1"]), sb(o=p["sl"]), sb(o=at("v", 16))]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), bad
    assert dd(A=1 << 10, T=(1 << 10) + 1) == _lib.EUNSUPPORTED and dd(A=1 << 10, T=1 << 10, D=3) == _lib.EUNSUPPORTED
    assert sb(A=(1 << 20) + 1, T=1, sl=None) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for key, val in (("g", 7 + 7j), ("st", 9.0), ("o", 3 + 3j), ("v", 2 + 1j), ("m", 1 - 1j), ("w", 1.5)):
        assert bool((t[key] == val).all()), key
    # and the valid corners next to them: T == 1 without slot, no weights, no stats, no rotation, no input, in place, n == 0
    assert dd(T=1, sl=None, w=None, st=None, ref=-1) == 0 and sb(T=1, sl=None, v=None) == 0 and sb(o=p["v"], dirs=0) == 0
    assert dd(n=0, a1=None, a2=None, sl=None, v=None, m=None, w=None, T=1) == 0
    assert sb(n=0, v=None, o=None, a1=None, a2=None, m=None) == 0
    ctx.synchronize()


# ---- peel on a small imager ------------------------------------------------------------------------------------------------------
def peel_setup(ctx, kind, seed):
    """the observation of test_gpu_gaincal's selfcal tests, plus one bright component outside the field with its own gains:
    vis = g0 predict(model) g0^H + g1 dft_predict(component) g1^H"""
    import gridhip
    import torch
    from test_gpu_gaincal import NANT, THETA, LAM, observation
    from test_gpu_weights import make_imager
    uvw, a1, a2, sl, model, gt, aw, wt = observation(kind, seed)
    rng = np.random.default_rng(seed + 1000)
    g1 = (1 + 0.2 * rng.normal(size=(2, NANT))) * np.exp(1j * rng.uniform(-1, 1, (2, NANT)))
    im = make_imager(ctx, kind, THETA, LAM, uvw, aw)
    s = dict(im=im, dm=dev(model), d1=dev(a1), d2=dev(a2), dsl=dev(sl), dwt=dev(wt), nant=NANT, gt=np.stack([gt, g1]))
    comps = gridhip.components(dev(np.array([1.5 * THETA])), dev(np.array([-1.2 * THETA])), dev(np.array([6.0])))
    off = ctx.dft_predict(tuple(dev(x) for x in uvw), comps)  # (THETA / 2 is the edge of the field)
    s["pred"] = im.predict(s["dm"]).clone()
    s["vis"] = (ctx.apply_gains(dev(gt), s["pred"], s["d1"], s["d2"], slot=s["dsl"], inverse=False)[0]
                + ctx.apply_gains(dev(g1), off, s["d1"], s["d2"], slot=s["dsl"], inverse=False)[0])
    s["rows"] = torch.stack([torch.zeros_like(off), off]).contiguous()  # row 0 is the peel's to write
    return s


@pytest.mark.parametrize("kind", ["simple", "aw"])
def test_peel_is_predict_ddcal_subtract_apply(ctx, kind):
    import torch
    s = peel_setup(ctx, kind, 16)
    im, dm, vis, d1, d2, dsl, dwt, nant = (s[k] for k in ("im", "dm", "vis", "d1", "d2", "dsl", "dwt", "nant"))
    # (a fixed number of iterations, far past convergence: a stop on rel would let the order of the atomic sums move the count)
    kw = dict(slot=dsl, nslots=2, weights=dwt, niter=150, tol=0.0)
    # the calls it replaces
    rows0 = s["rows"].clone()
    im.predict(dm, out=rows0[0])
    _, _, worst = R.ddcal(host(vis), host(rows0), host(d1), host(d2), nant, slot=host(dsl), T=2, wt=host(dwt), niter=150, tol=0.0)
    assert worst > 1e-6
    g0, st0 = ctx.ddcal(vis, rows0, d1, d2, nant, **kw)
    sub = ctx.dd_subtract(g0, rows0, d1, d2, slot=dsl, directions=[1], vis=vis)
    v0, w0 = ctx.apply_gains(g0[0], sub, d1, d2, slot=dsl, weights=dwt)
    rows1 = s["rows"].clone()
    g1, v1, w1, st1 = im.peel(dm, vis, rows1, d1, d2, nant, **kw)
    G0, G1, V0, V1, W0, W1, S0, S1 = (host(x) for x in (g0, g1, v0, v1, w0, w1, st0, st1))
    scale = np.abs(G0).max()
    print(f"{kind}: gains {np.abs(G1 - G0).max() / scale:.2e} vis {np.abs(V1 - V0).max() / np.abs(V0).max():.2e} stats {S1}")
    assert G1.shape == (2, 2, nant) and np.array_equal(host(rows1)[1], host(rows0)[1])
    assert np.abs(host(rows1)[0] - host(rows0)[0]).max() <= 1e-12 * np.abs(host(rows0)[0]).max()  # (the same prediction)
    assert np.abs(G1 - G0).max() <= TOL * scale and np.abs(V1 - V0).max() <= 1e-9 * np.abs(V0).max()
    assert np.allclose(W1, W0, rtol=1e-9, atol=0) and np.array_equal(S1[[0, 4, 5, 6, 7]], S0[[0, 4, 5, 6, 7]])
    assert S1[0] == 150 and S1[7] == 0
    # the image of the peeled stream is closer to that of the uncorrupted field than plain selfcal's is
    _, vs, _, _ = im.selfcal(dm, vis, d1, d2, nant, **kw)
    clean_img, self_img, peel_img = (host(im.cycle(x)) for x in (s["pred"], vs, v1))
    e_self, e_peel = np.abs(self_img - clean_img).max(), np.abs(peel_img - clean_img).max()
    print(f"{kind}: max |image - field image|: selfcal {e_self:.3e}, peel {e_peel:.3e}, ratio {e_peel / e_self:.3e}")
    assert e_peel / e_self < 1
    # a second call takes no memory
    out, wout = torch.empty_like(vis), torch.empty_like(dwt)
    im.peel(dm, vis, rows1, d1, d2, nant, gains=g1, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    im.peel(dm, vis, rows1, d1, d2, nant, gains=g1, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    im.close()


def test_peel_with_one_direction_is_selfcal(ctx):
    s = peel_setup(ctx, "simple", 19)
    im, dm, vis, d1, d2, dsl, dwt, nant = (s[k] for k in ("im", "dm", "vis", "d1", "d2", "dsl", "dwt", "nant"))
    kw = dict(slot=dsl, nslots=2, weights=dwt, niter=20, tol=0.0)
    g0, v0, w0, st0 = (host(x) for x in im.selfcal(dm, vis, d1, d2, nant, **kw))
    g1, v1, w1, st1 = (host(x) for x in im.peel(dm, vis, s["rows"][:1].clone(), d1, d2, nant, **kw))
    assert np.abs(g1[0] - g0).max() <= TOL * np.abs(g0).max() and np.abs(v1 - v0).max() <= 1e-9 * np.abs(v0).max()
    assert np.allclose(w1, w0, rtol=1e-9, atol=0) and np.array_equal(st1[[0, 4, 5, 6, 7]], st0[[0, 4, 5, 6, 7]])
    im.close()


def test_a_captured_peel_replays_to_the_eager_result(ctx):
    import torch
    s = peel_setup(ctx, "simple", 17)
    im, dm, vis, d1, d2, dsl, dwt, nant, rows = (s[k] for k in ("im", "dm", "vis", "d1", "d2", "dsl", "dwt", "nant", "rows"))
    kw = dict(slot=dsl, nslots=2, weights=dwt, niter=60, tol=0.0)
    eager = [host(x) for x in im.peel(dm, vis, rows, d1, d2, nant, **kw)]
    out, wout = torch.empty_like(vis), torch.empty_like(dwt)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        im.peel(dm, vis, rows, d1, d2, nant, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        g, _, _, stats = im.peel(dm, vis, rows, d1, d2, nant, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    for _ in range(2):
        g.fill_(7.0), out.fill_(7.0), wout.fill_(7.0), stats.fill_(7.0), rows[0].fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        G, V, W, S = host(g), host(out), host(wout), host(stats)
        assert np.abs(G - eager[0]).max() <= TOL * np.abs(eager[0]).max()
        assert np.abs(V - eager[1]).max() <= 1e-9 * np.abs(eager[1]).max() and np.allclose(W, eager[2], rtol=1e-9, atol=0)
        assert np.array_equal(S[[0, 4, 5, 6, 7]], eager[3][[0, 4, 5, 6, 7]]) and S[0] == 60
    im.close()


def test_peel_refusals(ctx):
    """gridhip_imager_peel_dev on a live imager, through the C ABI: GRIDHIP_EINVAL and the outputs stay as they were given."""
    import torch
    from gridhip import _lib
    from test_gpu_gaincal import NANT, THETA, LAM, observation
    from test_gpu_weights import make_imager
    lib = _lib.load()
    uvw, a1, a2, sl, model, _, _, wt = observation("simple", 18)
    im = make_imager(ctx, "simple", THETA, LAM, uvw, None)
    n, A, T, D = len(a1), NANT, 2, 2
    full = lambda shape, val, dt=torch.complex128: torch.full(shape, val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(model=dev(model), a1=dev(a1), a2=dev(a2), sl=dev(sl), w=dev(wt), v=full((n,), 2 + 1j), m=full((D * n,), 1 - 1j),
             g=full((D * T * A + 1,), 7 + 7j), st=full((8,), 9.0, torch.float64), o=full((n,), 3 + 3j),
             wo=full((n,), 4.0, torch.float64))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731

    def pl(h=im._h, model=p["model"], v=p["v"], A=A, T=T, D=D, a1=p["a1"], a2=p["a2"], sl=p["sl"], w=p["w"], mode=0, ref=0,
           warm=0, niter=3, tol=0.0, m=p["m"], g=p["g"], o=p["o"], wo=p["wo"], st=p["st"]):
        return lib.gridhip_imager_peel_dev(h, model, v, A, T, D, a1, a2, sl, w, mode, ref, warm, niter, tol, m, g, o, wo, st)

    torch.cuda.synchronize()
    bad = [pl(h=None), pl(model=None), pl(v=None), pl(A=1), pl(T=0), pl(D=0), pl(D=9), pl(sl=None), pl(a1=None), pl(a2=None),
           pl(m=None), pl(g=None), pl(o=None), pl(niter=-1), pl(tol=-1.0), pl(tol=float("nan")), pl(mode=2), pl(ref=A),
           pl(g=p["v"]), pl(g=p["m"]), pl(g=p["w"]), pl(o=p["g"]), pl(wo=p["g"]), pl(o=p["m"]), pl(o=at("m", 16 * (D * n - 1))),
           pl(o=p["a2"]), pl(wo=p["sl"]), pl(o=at("v", 16)), pl(wo=at("w", 8)), pl(o=p["w"]), pl(wo=p["o"]),
           pl(m=p["v"]), pl(m=p["w"]), pl(m=p["a1"]), pl(wo=p["m"]), pl(st=p["m"])]
    assert bad == [_lib.EINVAL] * len(bad), bad
    assert pl(A=1 << 10, T=(1 << 10) + 1) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for key, val in (("g", 7 + 7j), ("st", 9.0), ("o", 3 + 3j), ("wo", 4.0), ("v", 2 + 1j), ("m", 1 - 1j)):
        assert bool((t[key] == val).all()), key
    assert np.array_equal(host(t["w"]), wt)
    # and the valid corners next to them: no weights, no corrected weights, no stats, no rotation; in place
    assert pl(w=None, wo=None, st=None, ref=-1) == 0 and pl(o=p["v"], wo=p["w"]) == 0
    ctx.synchronize()
    assert t["g"][D * T * A] == 7 + 7j and not bool((t["m"][:n] == 1 - 1j).any()) and bool((t["m"][n:] == 1 - 1j).all())
    im.close()
