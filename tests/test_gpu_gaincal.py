"""Gain calibration on the device (gridhip_gaincal*, gridhip_apply_gains*, gridhip_imager_selfcal_dev) against the numpy
restatement tests/gaincal_ref.py, at fixed niter and tol = 0 so that rounding cannot move the stop.

Tolerances.  Gains: 1e-10 of the largest |g| - the project's tolerance for sums that meet in fp64 atomics; these have at
most a few thousand terms per antenna.  The integer entries of stats (iterations, n_used, n_flagged, n_dropped,
n_unsolved): exact.  chi^2 and chi^2 at g = 1: 1e-9 relative.  The last rel: it is sqrt(sum |g' - g|^2 / sum |g'|^2), and a perturbation of every gain by
e = 1e-10 max|g| moves the numerator's root by at most 2 e sqrt(cells) and the denominator's by at most e sqrt(cells), so
rel moves by at most (2 + rel) e max|g| / rms|g'| - REL_TOL allows 1e-9 + 1e-9 rel, max|g| / rms|g'| being below 3 in
every case here."""
import ctypes as C

import numpy as np
import pytest

import gaincal_ref as R
from test_gaincal_host import corrupted
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
    V, M = np.asarray(V, dtype=c128), np.asarray(M, dtype=c128)
    wt = None if wt is None else np.asarray(wt, dtype=f64)
    if form == "host":
        g, st = ctx.gaincal(V, M, a1, a2, A, slot=slot, weights=wt, gains=None if gains is None else gains.copy(), **kw)
        return g, st
    g, st = ctx.gaincal(dev(V), dev(M), dev(a1), dev(a2), A, slot=dev(slot), weights=dev(wt),
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


def both(ctx, what, V, M, a1, a2, A, forms=("dev", "host"), **kw):
    ref_kw = {k: v for k, v in kw.items() if k != "gains"}
    gr, sr = R.gaincal(V, M, a1, a2, A, gains=kw.get("gains"), **{"niter": 4, "tol": 0.0, **ref_kw})
    out = None
    for form in forms:
        g, st = solve(ctx, V, M, a1, a2, A, form=form, **kw)
        agree(f"{what} [{form}]", g, st, gr, sr)
        out = g, st
    return out, (gr, sr)


# ---- smallest shapes -------------------------------------------------------------------------------------------------------
def test_one_visibility_two_antennas(ctx):
    both(ctx, "A=2 n=1", [2 + 1j], [1 - 1j], [0], [1], 2)
    both(ctx, "A=2 n=1 swapped, weighted", [2 + 1j], [1 - 1j], [1], [0], 2, wt=[0.25], refant=1)


def test_three_visibilities_three_antennas(ctx):
    V, M = np.array([2 + 1j, 1 - 3j, -1 + 0.5j]), np.array([1 + 1j, 2 + 0j, 0.5 - 1j])
    for niter in (1, 2, 5):
        both(ctx, f"A=3 n=3 niter={niter}", V, M, [0, 0, 1], [1, 2, 2], 3, wt=[1.0, 2.0, 0.5], niter=niter, refant=-1)


@pytest.mark.parametrize("mode", [0, 1])
def test_every_baseline_three_intervals(ctx, mode):
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(5), 7, 3, noise=0.05)
    both(ctx, f"A=7 T=3 mode={mode}", V, M, a1, a2, 7, slot=sl, T=3, wt=w, mode=mode, niter=9, refant=3)


def test_no_visibilities_and_no_iterations(ctx):
    e = np.zeros(0)
    (g, st), _ = both(ctx, "n=0", e.astype(c128), e.astype(c128), e.astype(i64), e.astype(i64), 3, niter=3)
    assert np.all(g == 1) and st[7] == 3 and st[0] == 3 and st[1] == 0
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(6), 4, 2)
    (g, st), _ = both(ctx, "niter=0", V, M, a1, a2, 4, slot=sl, T=2, wt=w, niter=0)
    assert np.all(g == 1) and st[0] == 0 and st[7] == 8 and st[4] == len(V)
    warm = (np.arange(8).reshape(2, 4) - 2.5j + 1).astype(c128)
    (g, st), _ = both(ctx, "niter=0 warm", V, M, a1, a2, 4, slot=sl, T=2, wt=w, niter=0, gains=warm)
    assert np.array_equal(g, warm)


# ---- degenerate data -------------------------------------------------------------------------------------------------------
def test_missing_antennas_intervals_refant_autos_and_indices_out_of_range(ctx):
    rng = np.random.default_rng(7)
    A, T = 6, 4
    a1, a2, sl, V, M, w, _ = corrupted(rng, A, T, noise=0.05)
    keep = (a1 != 4) & (a2 != 4) & (sl != 2) & ~((sl == 1) & ((a1 == 0) | (a2 == 0)))  # antenna 4, interval 2: no data;
    a1, a2, sl, V, M, w = (x[keep] for x in (a1, a2, sl, V, M, w))                      # refant 0 unsolved in interval 1
    warm = (1 + 0.2 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-1, 1, (T, A)))
    for gains in (None, warm):
        (g, st), (gr, _) = both(ctx, f"missing data warm={gains is not None}", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6,
                                gains=gains)
        start = np.ones((T, A)) if gains is None else warm
        assert st[7] == T + A - 1 + 1  # antenna 4 everywhere, the rest of interval 2, refant 0 in interval 1
        assert np.array_equal(g[:, 4], start[:, 4]) and np.array_equal(g[2], start[2]) and g[1, 0] == start[1, 0]
        assert np.all(g[[0, 3], 0].imag == 0) and np.all(g[[0, 3], 0].real > 0)
    # autocorrelations and indices out of range on both sides: counted, and the other gains are those without them
    extra = np.array([[2, 2, 0], [5, 5, 3], [-1, 2, 0], [A, 2, 0], [1, -1, 0], [1, A, 3], [0, 1, -1], [0, 1, T]])
    n0, ne = len(a1), len(extra)
    a1x, a2x, slx = (np.concatenate([x, extra[:, i]]) for i, x in enumerate((a1, a2, sl)))
    Vx, Mx, wx = np.concatenate([V, np.full(ne, 5 + 5j)]), np.concatenate([M, np.full(ne, 1 - 2j)]), np.concatenate([w, np.ones(ne)])
    order = rng.permutation(n0 + ne)
    (g0, st0), _ = both(ctx, "without the dropped", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6, forms=("dev",))
    (g1, st1), _ = both(ctx, "with the dropped", Vx[order], Mx[order], a1x[order], a2x[order], A, slot=slx[order], T=T,
                        wt=wx[order], niter=6)
    assert st1[6] == ne and st0[6] == 0 and st1[4] == st0[4] == n0
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max()


def test_flagged_nan_and_inf_contribute_exactly_nothing(ctx):
    rng = np.random.default_rng(8)
    a1, a2, sl, V, M, w, _ = corrupted(rng, 5, 2, noise=0.05)
    n = len(a1)
    (g0, st0), _ = both(ctx, "clean", V, M, a1, a2, 5, slot=sl, T=2, wt=w, niter=6, forms=("dev",))
    bad = rng.choice(n, 12, replace=False)
    Vx, Mx, wx = np.tile(V, 2), np.tile(M, 2), np.concatenate([w, np.zeros(n)])  # every visibility again, flagged ...
    wx[n + bad[:4]], wx[n + bad[4:8]] = np.nan, -1.0
    Vx[n + bad] = [np.nan, np.inf, -np.inf, np.nan + 1j * np.inf] * 3            # ... and carrying NaN and Inf
    Mx[n + bad[::2]] = np.nan
    Mx[n + bad[1::2]] = np.inf
    order = rng.permutation(2 * n)
    (g1, st1), _ = both(ctx, "flagged", Vx[order], Mx[order], np.tile(a1, 2)[order], np.tile(a2, 2)[order], 5,
                        slot=np.tile(sl, 2)[order], T=2, wt=wx[order], niter=6)
    assert st1[5] == n and np.array_equal(st1[[0, 4, 6, 7]], st0[[0, 4, 6, 7]])
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max() and np.isfinite(st1).all()


# ---- chunking --------------------------------------------------------------------------------------------------------------
def stream(rng, n, A, T, order="time"):
    a1 = rng.integers(0, A, n)
    a2 = (a1 + rng.integers(1, A, n)) % A
    sl = rng.integers(0, T, n)
    if order == "time":
        sl = np.sort(sl)
    M = rng.normal(size=n) + 1j * rng.normal(size=n) + 3
    gt = (1 + 0.2 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-1, 1, (T, A)))
    V = gt[sl, a1] * M * np.conj(gt[sl, a2]) + 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return a1, a2, sl, V, M, rng.uniform(0.5, 2, n)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_around_one_chunk(ctx, n):
    a1, a2, sl, V, M, w = stream(np.random.default_rng(n), n, 8, 3)
    both(ctx, f"n={n}", V, M, a1, a2, 8, slot=sl, T=3, wt=w, niter=3, forms=("dev",))


def test_interval_change_on_a_chunk_boundary_and_inside_a_step(ctx):
    rng = np.random.default_rng(9)
    n = 3 * CHUNK
    a1, a2, _, V, M, w = stream(rng, n, 8, 1)
    for what, sl in (("on the boundary", np.repeat([0, 1, 2], CHUNK)),
                     ("one before and one after", np.repeat([0, 1, 2], [CHUNK - 1, CHUNK + 2, CHUNK - 1])),
                     ("every visibility", np.arange(n) % 3)):
        both(ctx, f"interval change {what}", V, M, a1, a2, 8, slot=sl, T=3, wt=w, niter=3, forms=("dev",))


def test_unordered_slots_agree_with_the_sorted_stream(ctx):
    rng = np.random.default_rng(10)
    n, A, T = 2 * CHUNK + 77, 16, 5
    a1, a2, sl, V, M, w = stream(rng, n, A, T)
    (g0, _), _ = both(ctx, "sorted", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=4, forms=("dev",))
    o = rng.permutation(n)
    (g1, _), _ = both(ctx, "permuted", V[o], M[o], a1[o], a2[o], A, slot=sl[o], T=T, wt=w[o], niter=4, forms=("dev",))
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max()


def test_ranges_of_several_chunks(ctx):
    """More chunks than the launch has work-groups (five per CU at the most): a work-group then takes a contiguous range of
    several chunks - the only size at which that path runs.  One iteration keeps the numpy reference at a few seconds."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = (5 * ncu + 1) * CHUNK + 5
    a1, a2, sl, V, M, w = stream(np.random.default_rng(11), n, 4, 3)
    both(ctx, f"n={n}", V, M, a1, a2, 4, slot=sl, T=3, wt=w, niter=1, forms=("dev",))


# ---- the LDS table's edges and the limit on A * T ---------------------------------------------------------------------------
@pytest.mark.parametrize("A", [512, 513])
def test_lds_table_edges(ctx, A):
    a1, a2, sl, V, M, w = stream(np.random.default_rng(A), 3 * CHUNK, A, 2)
    a1[:4], a2[:4] = [0, A - 1, A - 2, 0], [A - 1, 0, A - 1, 1]  # the table's last rows are used
    both(ctx, f"A={A}", V, M, a1, a2, A, slot=sl, T=2, wt=w, niter=3, forms=("dev",))


def test_table_limit(ctx):
    import torch
    A, T = 512, 4096  # A * T = 2^21, the stated limit
    rng = np.random.default_rng(12)
    n = 2000
    a1, a2, sl, V, M, w = stream(rng, n, A, T)
    sl[:2], a1[:2], a2[:2] = [0, T - 1], [0, A - 1], [A - 1, 0]
    both(ctx, "A*T at the limit", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=2, forms=("dev",))
    g = torch.full((T, A + 1), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    from gridhip import GridHipError, _lib
    with pytest.raises(GridHipError) as ei:
        ctx.gaincal(dev(V), dev(M), dev(a1), dev(a2), A + 1, slot=dev(sl), nslots=T, gains=g)
    assert ei.value.code == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((g == 7 + 7j).all())
    with pytest.raises(GridHipError) as ei:
        ctx.apply_gains(g, dev(V), dev(a1), dev(a2), slot=dev(sl))
    assert ei.value.code == _lib.EUNSUPPORTED


# ---- the stop on the device ------------------------------------------------------------------------------------------------
def test_stop_on_the_device(ctx):
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(139), 7, 3, noise=0.02)
    tol, hist = 1e-8, []
    gr, sr = R.gaincal(V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=100, tol=tol, history=hist)
    k = len(hist)
    # (the seed was chosen so: rounding cannot move the stop)
    assert k < 100 and hist[-1] <= tol / 2 and hist[-2] >= 2 * tol and sr[0] == k
    g, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=100, tol=tol)
    agree("stopped", g, st, gr, sr)
    assert st[0] == k
    # exactly k iterations without a stop rule give the same gains: the 100 - k later launches changed nothing
    g2, st2 = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=k, tol=0.0)
    assert st2[0] == k and np.abs(g2 - g).max() <= TOL * np.abs(g).max() and abs(st2[1] - st[1]) <= 1e-9


def test_warm_start_reproduces_a_split_solve(ctx):
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(14), 6, 2, noise=0.05)
    k = 4  # even: the second half then averages on the same iterations as the whole
    whole, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=2 * k, refant=-1)
    half, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1)
    rest, st = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1, gains=half)
    assert st[0] == k and np.abs(rest - whole).max() <= TOL * np.abs(whole).max()
    both(ctx, "warm", V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, gains=half)


# ---- apply -----------------------------------------------------------------------------------------------------------------
def test_apply_both_directions_in_place_and_unusable_gains(ctx):
    import torch
    rng = np.random.default_rng(15)
    n, A, T = CHUNK + 33, 6, 3
    a1, a2, sl, V, M, w = stream(rng, n, A, T)
    a1[:6], a2[:6], sl[:6] = [-1, A, 0, 0, 1, 1], [0, 1, -1, A, 2, 1], [0, 0, 0, 0, T, 0]  # out of range; an autocorrelation
    g = (1 + 0.3 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-2, 2, (T, A)))
    g[1, 2], g[2, 3], g[0, 4] = 0, np.nan, np.inf + 0j
    w[7] = 0.0
    for inverse in (True, False):
        vr, wr = R.apply_gains(g, V, a1, a2, slot=sl, wt=w, inverse=inverse)
        for form in ("host", "dev"):
            if form == "host":
                vo, wo = ctx.apply_gains(g, V, a1, a2, slot=sl, weights=w, inverse=inverse)
            else:
                vo, wo = (host(x) for x in ctx.apply_gains(dev(g), dev(V), dev(a1), dev(a2), slot=dev(sl), weights=dev(w),
                                                           inverse=inverse))
            fin = np.isfinite(vr)
            assert np.array_equal(fin, np.isfinite(vo))
            assert np.abs(vo[fin] - vr[fin]).max() <= 1e-12 * np.abs(vr[fin]).max()
            assert np.allclose(wo, wr, rtol=1e-14, atol=0, equal_nan=True)
            if inverse:
                unusable = ~((a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (sl >= 0) & (sl < T))
                ok = ~unusable
                unusable[ok] = ~np.isfinite(g[sl[ok], a1[ok]] * g[sl[ok], a2[ok]]) | (g[sl[ok], a1[ok]] * g[sl[ok], a2[ok]] == 0)
                assert unusable.sum() > 20 and np.array_equal(vo[unusable], V[unusable])
                assert np.all(wo[unusable] == 0.0) and not np.signbit(wo[unusable]).any()
    # without weights: ones; in place; and correcting what was corrupted gives the input back
    good = np.where(np.isfinite(g) & (g != 0), g, 1.0)
    dv, dw = dev(V), dev(w)
    v0, _ = ctx.apply_gains(dev(good), dv, dev(a1), dev(a2), slot=dev(sl), inverse=False, out=dv)
    assert v0 is dv
    vb, wb = ctx.apply_gains(dev(good), dv, dev(a1), dev(a2), slot=dev(sl), weights=dw, out=dv, weights_out=dw)
    assert vb is dv and wb is dw
    torch.cuda.synchronize()
    assert np.abs(host(dv) - V).max() <= 1e-12 * np.abs(V).max()
    _, wr = R.apply_gains(good, V, a1, a2, slot=sl, wt=w)
    assert np.allclose(host(dw), wr, rtol=1e-14, atol=0)
    _, w1 = ctx.apply_gains(good, V, a1, a2, slot=sl)
    assert np.allclose(w1, R.apply_gains(good, V, a1, a2, slot=sl)[1], rtol=1e-14, atol=0)


def both_forms(ctx, name, scalars_and_arrays):
    """gridhip_<name> on numpy arrays and gridhip_<name>_dev on device copies of them, through the C ABI.  An argument is a
    scalar, None, or a numpy array; an array that occurs twice (an output that is its own input) is one array on the
    device too.  -> ({id: the host array after the call}, {id: the device copy after the call, brought back})"""
    import torch
    from gridhip._marshal import device
    lib, h = ctx._lib, ctx._h
    arrays = {id(a): a for a in scalars_and_arrays if isinstance(a, np.ndarray)}
    hst = {k: a.copy() for k, a in arrays.items()}
    dvc = {k: to_dev(a if a.size else np.zeros(1, a.dtype)) for k, a in arrays.items()}  # (an empty tensor has no address)
    hp = lambda a: C.c_void_p(hst[id(a)].ctypes.data) if isinstance(a, np.ndarray) else a  # noqa: E731
    dp = lambda a: C.c_void_p(dvc[id(a)].data_ptr()) if isinstance(a, np.ndarray) else a  # noqa: E731
    assert getattr(lib, "gridhip_" + name)(h, *[hp(a) for a in scalars_and_arrays]) == 0
    device().bind(ctx)
    assert getattr(lib, "gridhip_" + name + "_dev")(h, *[dp(a) for a in scalars_and_arrays]) == 0
    torch.cuda.synchronize()
    return hst, {k: host(t).reshape(-1)[:arrays[k].size].reshape(arrays[k].shape) for k, t in dvc.items()}


@pytest.mark.parametrize("n", [0, 1, 257])  # none, one, one work-group and one
def test_apply_host_and_device_forms_give_the_same_bits(ctx, n):
    """Every staging branch of gridhip_apply_gains: slot, wt_in and wt_out present and null, out of place and in place.
    The correction is one rounded expression per visibility, so the two forms give the same bits; the restatement rounds
    its products in another order, so it holds within the bounds of the test above (1e-12 of the largest, 1e-14 relative)."""
    rng = np.random.default_rng(300 + n)
    A, T = 3, 2
    a1, a2, sl, V, _, w = stream(rng, n, A, T)
    g = (1 + 0.3 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-2, 2, (T, A)))
    for slot in (sl, None):
        gg = g if slot is not None else g[:1].copy()
        for wt in (w, None):
            for want_wo in (True, False):
                for in_place in (False, True):
                    for inverse in (1, 0):
                        vin = V.copy()
                        vout = vin if in_place else np.full(n, 7 - 7j)
                        wi = None if wt is None else wt.copy()
                        wo = None if not want_wo else wi if in_place and wi is not None else np.full(n, 7.0)
                        hst, dvc = both_forms(ctx, "apply_gains", [n, A, len(gg), a1, a2, slot, gg, inverse, vin, wi, vout, wo])
                        what = (n, slot is not None, wt is not None, want_wo, in_place, inverse)
                        for k in hst:
                            assert hst[k].tobytes() == dvc[k].tobytes(), what
                        for x in (a1, a2, gg) + (() if in_place else (vin,)):
                            assert hst[id(x)].tobytes() == x.tobytes(), what  # inputs as they were
                        vr, wr = R.apply_gains(gg, V, a1, a2, slot=slot, wt=wt, inverse=bool(inverse))
                        if n:
                            assert np.abs(hst[id(vout)] - vr).max() <= 1e-12 * np.abs(vr).max(), what
                        if wo is not None:
                            assert np.allclose(hst[id(wo)], wr, rtol=1e-14, atol=0), what


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header, through the C ABI on device memory: GRIDHIP_EINVAL and the outputs as they were given."""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    n, A, T = 5, 3, 2
    t = dict(a1=to_dev(np.array([0, 0, 1, 0, 1], dtype=i64)), a2=to_dev(np.array([1, 2, 2, 1, 2], dtype=i64)),
             sl=to_dev(np.array([0, 0, 0, 1, 1], dtype=i64)), v=torch.full((2 * n,), 2 + 1j, dtype=torch.complex128, device="cuda:0"),
             m=torch.full((n,), 1 - 1j, dtype=torch.complex128, device="cuda:0"),
             w=torch.full((n,), 1.5, dtype=torch.float64, device="cuda:0"),
             g=torch.full((T * A + 1,), 7 + 7j, dtype=torch.complex128, device="cuda:0"),
             st=torch.full((8,), 9.0, dtype=torch.float64, device="cuda:0"),
             o=torch.full((n,), 3 + 3j, dtype=torch.complex128, device="cuda:0"),
             wo=torch.full((n,), 4.0, dtype=torch.float64, device="cuda:0"))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    h = ctx._h

    def gc(n=n, A=A, T=T, a1=p["a1"], a2=p["a2"], sl=p["sl"], v=p["v"], m=p["m"], w=p["w"], mode=0, ref=0, warm=0,
           niter=3, tol=0.0, g=p["g"], st=p["st"]):
        return lib.gridhip_gaincal_dev(h, n, A, T, a1, a2, sl, v, m, w, mode, ref, warm, niter, tol, g, st)

    def ap(n=n, A=A, T=T, a1=p["a1"], a2=p["a2"], sl=p["sl"], g=p["g"], inv=1, v=p["v"], w=p["w"], o=p["o"], wo=p["wo"]):
        return lib.gridhip_apply_gains_dev(h, n, A, T, a1, a2, sl, g, inv, v, w, o, wo)

    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    bad = [gc(n=-1), gc(A=1), gc(T=0), gc(sl=None), gc(a1=None), gc(a2=None), gc(v=None), gc(m=None), gc(g=None),
           gc(niter=-1), gc(tol=-1.0), gc(tol=float("nan")), gc(mode=2), gc(mode=-1), gc(ref=A), gc(g=p["v"]), gc(g=p["m"]),
           gc(g=p["w"]), gc(g=p["a1"]), gc(g=p["a2"]), gc(g=p["sl"]), gc(g=at("v", 16 * n - 8), v=p["v"]),
           ap(n=-1), ap(A=1), ap(T=0), ap(sl=None), ap(a1=None), ap(a2=None), ap(g=None), ap(v=None), ap(o=None), ap(inv=2),
           ap(inv=-1), ap(o=p["g"]), ap(wo=p["g"]), ap(o=p["a1"]), ap(wo=p["sl"]), ap(o=at("v", 16)), ap(wo=at("w", 8)),
           ap(o=p["w"]), ap(wo=p["o"])]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), bad
    assert gc(A=1 << 11, T=(1 << 10) + 1) == _lib.EUNSUPPORTED and ap(A=(1 << 21) + 1, T=1, sl=None) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for key, val in (("g", 7 + 7j), ("st", 9.0), ("o", 3 + 3j), ("wo", 4.0), ("v", 2 + 1j), ("w", 1.5)):
        assert bool((t[key] == val).all()), key
    # and the valid corners next to them: T == 1 without slot, no weights, no stats, no rotation, wt_out NULL, n == 0
    assert gc(T=1, sl=None, w=None, st=None, ref=-1) == 0 and ap(T=1, sl=None, w=None, wo=None) == 0
    assert gc(n=0, a1=None, a2=None, sl=None, v=None, m=None, w=None, T=1) == 0 and ap(n=0, v=None, o=None, a1=None, a2=None) == 0
    ctx.synchronize()


# ---- imagers ---------------------------------------------------------------------------------------------------------------
THETA, LAM, NPIX = 0.008, 2000, 16  # as the weights tests use: N = 16
NANT = 6


def observation(kind, seed, n=600):
    """baselines inside the grid, a point-source model, antenna pairs, two solution intervals, gains to recover"""
    from test_gpu_imager import aw_tables
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.4, 0.4, n) * LAM, rng.uniform(-0.4, 0.4, n) * LAM
    w = rng.uniform(-50, 50, n)
    p, q = np.triu_indices(NANT, 1)
    pick = rng.integers(0, len(p), n)
    a1, a2, sl = p[pick], q[pick], np.sort(rng.integers(0, 2, n))
    model = np.zeros((NPIX, NPIX))
    model[NPIX // 2 + 2, NPIX // 2 - 3] = 4.0
    gt = (1 + 0.2 * rng.normal(size=(2, NANT))) * np.exp(1j * rng.uniform(-1, 1, (2, NANT)))
    aw = None
    if kind == "aw":
        wk, wv, ak = aw_tables(3, 2, 9, NANT, 100.0, seed)
        aw = (wk, wv, ak, a1, a2)
    return (u, v, w), a1, a2, sl, model, gt, aw, rng.uniform(0.5, 2, n)


@pytest.mark.parametrize("kind", ["simple", "aw"])
def test_selfcal_is_predict_gaincal_apply(ctx, kind):
    import torch
    from test_gpu_weights import make_imager
    uvw, a1, a2, sl, model, gt, aw, wt = observation(kind, 16)
    im = make_imager(ctx, kind, THETA, LAM, uvw, aw)
    dm, d1, d2, dsl, dwt = dev(model), dev(a1), dev(a2), dev(sl), dev(wt)
    pred = im.predict(dm)
    vis = ctx.apply_gains(dev(gt), pred, d1, d2, slot=dsl, inverse=False)[0].clone()
    # (a fixed number of iterations, far past convergence: a stop on rel would let the order of the atomic sums move the count)
    kw = dict(slot=dsl, nslots=2, weights=dwt, niter=100, tol=0.0)
    # the calls it replaces
    g0, st0 = ctx.gaincal(vis, im.predict(dm), d1, d2, NANT, **kw)
    v0, w0 = ctx.apply_gains(g0, vis, d1, d2, slot=dsl, weights=dwt)
    g1, v1, w1, st1 = im.selfcal(dm, vis, d1, d2, NANT, **kw)
    G0, G1, V0, V1, W0, W1, S0, S1 = (host(x) for x in (g0, g1, v0, v1, w0, w1, st0, st1))
    scale = np.abs(G0).max()
    print(f"{kind}: gains {np.abs(G1 - G0).max() / scale:.2e} vis {np.abs(V1 - V0).max() / np.abs(V0).max():.2e} stats {S1}")
    assert np.abs(G1 - G0).max() <= TOL * scale and np.abs(V1 - V0).max() <= 1e-9 * np.abs(V0).max()
    assert np.allclose(W1, W0, rtol=1e-9, atol=0) and np.array_equal(S1[[0, 4, 5, 6, 7]], S0[[0, 4, 5, 6, 7]])
    assert S1[0] == 100 and S1[7] == 0 and S1[2] <= 1e-16 * S1[3]
    # the known gains come back up to the reference phase, and with them the dirty image's peak
    truth = gt * np.exp(-1j * np.angle(gt[:, :1]))
    reached = np.abs(G1 - truth).max()
    print(f"{kind}: gain error {reached:.2e}")
    assert reached < 1e-8
    clean_img, bad_img, cal_img = (host(im.cycle(x)) for x in (pred, vis, v1))
    peak = np.unravel_index(np.abs(clean_img).argmax(), clean_img.shape)
    assert abs(bad_img[peak] - clean_img[peak]) > 1e-3 * abs(clean_img[peak])
    # (the corrected stream is the prediction to the accuracy the solve reached - a gain error e moves g_p conj(g_q) by
    # about 2 e |g|, |g| within 0.4 .. 1.6 here: 10 e relative at the most - plus the 1e-10 of the imager's own fp64-atomic
    # sums)
    print(f"{kind}: peak {clean_img[peak]:.6e} corrupted {bad_img[peak]:.6e} corrected {cal_img[peak]:.6e}")
    assert abs(cal_img[peak] - clean_img[peak]) <= (10 * reached + TOL) * abs(clean_img[peak])
    # a second call takes no memory
    out, wout = torch.empty_like(vis), torch.empty_like(dwt)
    im.selfcal(dm, vis, d1, d2, NANT, gains=g1, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    im.selfcal(dm, vis, d1, d2, NANT, gains=g1, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    im.close()


def test_a_captured_selfcal_replays_to_the_eager_result(ctx):
    import torch
    from test_gpu_weights import make_imager
    uvw, a1, a2, sl, model, gt, aw, wt = observation("simple", 17)
    im = make_imager(ctx, "simple", THETA, LAM, uvw, None)
    dm, d1, d2, dsl, dwt = dev(model), dev(a1), dev(a2), dev(sl), dev(wt)
    vis = ctx.apply_gains(dev(gt), im.predict(dm), d1, d2, slot=dsl, inverse=False)[0].clone()
    kw = dict(slot=dsl, nslots=2, weights=dwt, niter=60, tol=0.0)
    eager = [host(x) for x in im.selfcal(dm, vis, d1, d2, NANT, **kw)]
    out, wout = torch.empty_like(vis), torch.empty_like(dwt)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        im.selfcal(dm, vis, d1, d2, NANT, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        g, _, _, stats = im.selfcal(dm, vis, d1, d2, NANT, out=out, weights_out=wout, **kw)
    torch.cuda.synchronize()
    for _ in range(2):
        g.fill_(7.0), out.fill_(7.0), wout.fill_(7.0), stats.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        G, V, W, S = host(g), host(out), host(wout), host(stats)
        assert np.abs(G - eager[0]).max() <= TOL * np.abs(eager[0]).max()
        assert np.abs(V - eager[1]).max() <= 1e-9 * np.abs(eager[1]).max() and np.allclose(W, eager[2], rtol=1e-9, atol=0)
        assert np.array_equal(S[[0, 4, 5, 6, 7]], eager[3][[0, 4, 5, 6, 7]]) and S[0] == 60
    im.close()


def test_selfcal_refusals(ctx):
    """gridhip_imager_selfcal_dev on a live imager, through the C ABI: every rule of the header is GRIDHIP_EINVAL (the table
    limit GRIDHIP_EUNSUPPORTED) and the outputs stay as they were given."""
    import torch
    from gridhip import _lib
    from test_gpu_weights import make_imager
    lib = _lib.load()
    uvw, a1, a2, sl, model, _, _, wt = observation("simple", 18)
    im = make_imager(ctx, "simple", THETA, LAM, uvw, None)
    n, A, T = len(a1), NANT, 2
    t = dict(model=dev(model), a1=dev(a1), a2=dev(a2), sl=dev(sl), w=dev(wt),
             v=torch.full((n,), 2 + 1j, dtype=torch.complex128, device="cuda:0"),
             g=torch.full((T * A + 1,), 7 + 7j, dtype=torch.complex128, device="cuda:0"),
             st=torch.full((8,), 9.0, dtype=torch.float64, device="cuda:0"),
             o=torch.full((n,), 3 + 3j, dtype=torch.complex128, device="cuda:0"),
             wo=torch.full((n,), 4.0, dtype=torch.float64, device="cuda:0"))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731

    def sc(h=im._h, model=p["model"], v=p["v"], A=A, T=T, a1=p["a1"], a2=p["a2"], sl=p["sl"], w=p["w"], mode=0, ref=0,
           warm=0, niter=3, tol=0.0, g=p["g"], o=p["o"], wo=p["wo"], st=p["st"]):
        return lib.gridhip_imager_selfcal_dev(h, model, v, A, T, a1, a2, sl, w, mode, ref, warm, niter, tol, g, o, wo, st)

    torch.cuda.synchronize()
    bad = [sc(h=None), sc(model=None), sc(v=None), sc(A=1), sc(T=0), sc(sl=None), sc(a1=None), sc(a2=None), sc(g=None),
           sc(o=None), sc(niter=-1), sc(tol=-1.0), sc(tol=float("nan")), sc(mode=2), sc(mode=-1), sc(ref=A), sc(g=p["v"]),
           sc(g=p["w"]), sc(g=p["a1"]), sc(g=p["sl"]), sc(o=p["g"]), sc(wo=p["g"]), sc(o=at("g", 16 * (T * A - 1))),
           sc(o=p["a2"]), sc(wo=p["sl"]), sc(o=at("v", 16)), sc(wo=at("w", 8)), sc(o=p["w"]), sc(wo=p["o"])]
    assert bad == [_lib.EINVAL] * len(bad), bad
    assert sc(A=1 << 11, T=(1 << 10) + 1) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for key, val in (("g", 7 + 7j), ("st", 9.0), ("o", 3 + 3j), ("wo", 4.0), ("v", 2 + 1j)):
        assert bool((t[key] == val).all()), key
    assert np.array_equal(host(t["w"]), wt)
    # and the valid corners next to them: no weights, no corrected weights, no stats, no rotation; in place
    assert sc(w=None, wo=None, st=None, ref=-1) == 0 and sc(o=p["v"], wo=p["w"]) == 0
    ctx.synchronize()
    assert not bool((t["g"][:T * A] == 7 + 7j).any()) and t["g"][T * A] == 7 + 7j
    im.close()
