"""Polarisation on the device (gridhip_jonescal*, gridhip_apply_jones*, gridhip_stokes*) against the numpy restatement
tests/jonescal_ref.py, at fixed niter and tol = 0 so that rounding cannot move the stop.  It mirrors test_gpu_gaincal.py.

Tolerances.  Gains: 1e-10 of the largest |G| entry - the project's tolerance for sums that meet in fp64 atomics (permuting
a stream moves the restatement's gains by 6e-16 of the largest entry at niter = 9: five orders of margin).  The integer
entries of stats: exact.  chi^2 and chi^2 at G = I: 1e-9 relative.  The last rel: 1e-9 + 1e-9 rel, by the argument in
test_gpu_gaincal.py's docstring (max|G| / rms|G'| is below 3 here too: the diagonals are near 1).  apply_jones: 1e-13 of
the sample's largest output entry for matrices of condition number <= 10 - the operation is a few dozen roundings scaled
by the conditioning - and the host and device forms give the same bits.  stokes: bit for bit."""
import ctypes as C

import numpy as np
import pytest

import jonescal_ref as J
from test_gpu_gaincal import both_forms
from test_gpu_imager import host, to_dev
from test_jonescal_host import polarised

pytestmark = pytest.mark.gpu

TOL = 1e-10
CHUNK = 4096  # the iteration kernel's chunk (GC_CHUNK, csrc/imaging.h)
c128, f64, i64 = np.complex128, np.float64, np.int64
MODES = {0: "full", 1: "diagonal", 2: "phase"}


def dev(x):
    return None if x is None else to_dev(x)


def solve(ctx, V, M, a1, a2, A, slot=None, T=1, wt=None, mode=0, refant=0, niter=4, tol=0.0, gains=None, form="dev"):
    """-> (gains, stats) as numpy arrays, by the device form (torch tensors) or the host form (numpy arrays)"""
    kw = dict(nslots=T, mode=MODES[mode], refant=None if refant < 0 else refant, niter=niter, tol=tol)
    a1, a2 = np.asarray(a1, dtype=i64), np.asarray(a2, dtype=i64)
    slot = None if slot is None else np.asarray(slot, dtype=i64)
    V, M = np.asarray(V, dtype=c128).reshape(-1, 2, 2), np.asarray(M, dtype=c128).reshape(-1, 2, 2)
    wt = None if wt is None else np.asarray(wt, dtype=f64)
    if form == "host":
        return ctx.jonescal(V, M, a1, a2, A, slot=slot, weights=wt, gains=None if gains is None else gains.copy(), **kw)
    g, st = ctx.jonescal(dev(V), dev(M), dev(a1), dev(a2), A, slot=dev(slot), weights=dev(wt),
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
    gr, sr = J.jonescal(V, M, a1, a2, A, gains=kw.get("gains"), **{"niter": 4, "tol": 0.0, **ref_kw})
    out = None
    for form in forms:
        g, st = solve(ctx, V, M, a1, a2, A, form=form, **kw)
        agree(f"{what} [{form}]", g, st, gr, sr)
        out = g, st
    return out, (gr, sr)


def eye(T, A):
    return np.broadcast_to(np.eye(2, dtype=c128), (T, A, 2, 2))


def mats(rng, *shape):
    return rng.normal(size=shape + (2, 2)) + 1j * rng.normal(size=shape + (2, 2))


# ---- smallest shapes -------------------------------------------------------------------------------------------------------
def test_one_visibility_two_antennas(ctx):
    V, M = [[2 + 1j, 0.5 - 1j], [-1 + 0.25j, 1 + 3j]], [[1 + 1j, 0.5j], [0.25 - 0.5j, 2 - 1j]]
    (g, st), _ = both(ctx, "A=2 n=1", [V], [M], [0], [1], 2)
    assert st[7] == 0  # one visibility makes both antennas solvable
    both(ctx, "A=2 n=1 swapped, weighted", [V], [M], [1], [0], 2, wt=[0.25], refant=1)


def test_three_visibilities_three_antennas(ctx):
    rng = np.random.default_rng(1)
    V, M = mats(rng, 3), mats(rng, 3)
    for niter in (1, 2, 5):  # odd and even averaging
        both(ctx, f"A=3 n=3 niter={niter}", V, M, [0, 0, 1], [1, 2, 2], 3, wt=[1.0, 2.0, 0.5], niter=niter, refant=-1)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_baseline_three_intervals(ctx, mode):
    rng = np.random.default_rng(5)
    a1, a2, sl, V, M, _ = polarised(rng, 7, 3, noise=0.05)
    both(ctx, f"A=7 T=3 mode={mode}", V, M, a1, a2, 7, slot=sl, T=3, wt=rng.uniform(0.5, 2, len(a1)), mode=mode, niter=9,
         refant=3)


def test_a_diagonal_solve_of_diagonal_data_is_gaincal_on_each_correlation(ctx):
    """Without off-diagonals the sums of [0][0] and [1][1] are gaincal's of the xx and the yy stream, so the two modules'
    walk, update and finish meet here.  No reference antenna: jonescal would rotate both diagonals by the phase of [0][0],
    gaincal each stream by its own."""
    rng = np.random.default_rng(5)
    a1, a2, sl, V, M, _ = polarised(rng, 7, 3, noise=0.05)
    V, M, w = V.copy(), M.copy(), rng.uniform(0.5, 2, len(a1))
    V[:, 0, 1] = V[:, 1, 0] = M[:, 0, 1] = M[:, 1, 0] = 0
    G, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, mode=1, refant=-1, niter=9)
    assert G.shape == (3, 7, 2, 2) and np.all(G[..., 0, 1] == 0) and np.all(G[..., 1, 0] == 0)
    for i, name in ((0, "xx"), (1, "yy")):
        g, sg = ctx.gaincal(dev(np.ascontiguousarray(V[:, i, i])), dev(np.ascontiguousarray(M[:, i, i])), dev(a1), dev(a2), 7,
                            slot=dev(sl), nslots=3, weights=dev(w), refant=None, niter=9, tol=0.0)
        g, sg = host(g), host(sg)
        eg = np.abs(G[..., i, i] - g).max() / np.abs(g).max()
        print(f"{name}: gains {eg:.2e}  ints {st[[0, 4, 5, 6, 7]]} / {sg[[0, 4, 5, 6, 7]]}")
        assert g.shape == (3, 7) and eg <= TOL, name
        assert np.array_equal(st[[0, 4, 5, 6, 7]], sg[[0, 4, 5, 6, 7]]), name


def test_no_visibilities_and_no_iterations(ctx):
    e = np.zeros(0)
    (g, st), _ = both(ctx, "n=0", np.zeros((0, 2, 2), c128), np.zeros((0, 2, 2), c128), e.astype(i64), e.astype(i64), 3, niter=3)
    assert np.array_equal(g, eye(1, 3)) and st[7] == 3 and st[0] == 3 and st[1] == 0
    rng = np.random.default_rng(6)
    a1, a2, sl, V, M, _ = polarised(rng, 4, 2)
    (g, st), _ = both(ctx, "niter=0", V, M, a1, a2, 4, slot=sl, T=2, niter=0)
    assert np.array_equal(g, eye(2, 4)) and st[0] == 0 and st[7] == 8 and st[4] == len(V)
    warm = mats(rng, 2, 4) + 2
    (g, st), _ = both(ctx, "niter=0 warm", V, M, a1, a2, 4, slot=sl, T=2, niter=0, gains=warm)
    assert g.tobytes() == warm.tobytes()  # the very bits
    for mode in (1, 2):
        (g, st), _ = both(ctx, f"niter=0 warm mode={mode}", V, M, a1, a2, 4, slot=sl, T=2, niter=0, gains=warm, mode=mode)
        off = g[..., [0, 1], [1, 0]]
        assert np.all(off == 0) and not np.signbit(off.real).any() and not np.signbit(off.imag).any()
        assert np.array_equal(g[..., [0, 1], [0, 1]], warm[..., [0, 1], [0, 1]])


# ---- unsolvable and unusual data -------------------------------------------------------------------------------------------
def test_missing_antennas_intervals_refant_autos_and_indices_out_of_range(ctx):
    rng = np.random.default_rng(7)
    A, T = 6, 4
    a1, a2, sl, V, M, _ = polarised(rng, A, T, noise=0.05)
    w = rng.uniform(0.5, 2, len(a1))
    keep = (a1 != 4) & (a2 != 4) & (sl != 2) & ~((sl == 1) & ((a1 == 0) | (a2 == 0)))  # antenna 4, interval 2: no data;
    a1, a2, sl, V, M, w = (x[keep] for x in (a1, a2, sl, V, M, w))                      # refant 0 unsolved in interval 1
    warm = mats(rng, T, A) * 0.2 + np.eye(2)
    for gains in (None, warm):
        (g, st), (gr, _) = both(ctx, f"missing data warm={gains is not None}", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6,
                                gains=gains)
        start = eye(T, A) if gains is None else warm
        assert st[7] == T + A - 1 + 1  # antenna 4 everywhere, the rest of interval 2, refant 0 in interval 1
        assert np.array_equal(g[:, 4], start[:, 4]) and np.array_equal(g[2], start[2]) and np.array_equal(g[1, 0], start[1, 0])
        assert np.all(g[[0, 3], 0, 0, 0].imag == 0) and np.all(g[[0, 3], 0, 0, 0].real > 0)
        # interval 1 is left unrotated: it is what the solve without a rotation gives
        g_free, _ = solve(ctx, V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6, gains=gains, refant=-1)
        assert np.abs(g[1] - g_free[1]).max() <= TOL * np.abs(g_free).max()
    # autocorrelations and indices out of range on each of p, q, t: counted, and the other gains are those without them
    extra = np.array([[2, 2, 0], [5, 5, 3], [-1, 2, 0], [A, 2, 0], [1, -1, 0], [1, A, 3], [0, 1, -1], [0, 1, T]])
    n0, ne = len(a1), len(extra)
    a1x, a2x, slx = (np.concatenate([x, extra[:, i]]) for i, x in enumerate((a1, a2, sl)))
    Vx, Mx = np.concatenate([V, np.full((ne, 2, 2), 5 + 5j)]), np.concatenate([M, np.full((ne, 2, 2), 1 - 2j)])
    wx = np.concatenate([w, np.ones(ne)])
    order = rng.permutation(n0 + ne)
    (g0, st0), _ = both(ctx, "without the dropped", V, M, a1, a2, A, slot=sl, T=T, wt=w, niter=6, forms=("dev",))
    (g1, st1), _ = both(ctx, "with the dropped", Vx[order], Mx[order], a1x[order], a2x[order], A, slot=slx[order], T=T,
                        wt=wx[order], niter=6)
    assert st1[6] == ne and st0[6] == 0 and st1[4] == st0[4] == n0
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max()


def test_models_that_leave_den_singular(ctx):
    rng = np.random.default_rng(17)
    A, T = 5, 2
    a1, a2, sl, V, M, _ = polarised(rng, A, T, noise=0.05)
    M1 = np.zeros_like(M)
    M1[:, 0, 0] = M[:, 0, 0]  # only XX non-zero
    warm = mats(rng, T, A) * 0.2 + np.eye(2)
    for mode in (0, 1):  # mode 1 is unsolved too: d11 = 0
        (g, st), _ = both(ctx, f"only XX, mode {mode}", V, M1, a1, a2, A, slot=sl, T=T, mode=mode, niter=4)
        assert st[7] == A * T and st[1] == 0 and np.array_equal(g, eye(T, A))
    (g, st), _ = both(ctx, "only XX, warm", V, M1, a1, a2, A, slot=sl, T=T, niter=4, gains=warm)
    assert st[7] == A * T and g.tobytes() == warm.tobytes()
    # YY alone is zero on the baselines of antenna 2: den stays regular through the other three correlations
    M2 = M.copy()
    M2[(a1 == 2) | (a2 == 2), 1, 1] = 0
    for mode in (0, 1, 2):
        both(ctx, f"YY zero on one antenna's baselines, mode {mode}", V, M2, a1, a2, A, slot=sl, T=T, mode=mode, niter=6)


def test_flagged_nan_and_inf_contribute_exactly_nothing(ctx):
    rng = np.random.default_rng(8)
    a1, a2, sl, V, M, _ = polarised(rng, 6, 3, noise=0.05)
    n = len(a1)  # 45
    w = rng.uniform(0.5, 2, n)
    (g0, st0), _ = both(ctx, "clean", V, M, a1, a2, 6, slot=sl, T=3, wt=w, niter=6, forms=("dev",))
    Vx, Mx, wx = np.tile(V, (2, 1, 1)), np.tile(M, (2, 1, 1)), np.concatenate([w, np.zeros(n)])  # every sample again, flagged
    wx[n + 4:n + 8], wx[n + 8:n + 12] = np.nan, -1.0
    bad = [np.nan, np.inf, -np.inf, complex(np.nan, np.inf)]
    for k in range(16):  # NaN and Inf in every one of the eight numbers, of the data and of the model, with each kind of weight
        i, j, part = (k >> 2) & 1, (k >> 1) & 1, k & 1
        z = Vx[n + k, i, j]
        Vx[n + k, i, j] = complex(bad[k % 3], z.imag) if part == 0 else complex(z.real, bad[k % 3])
        z = Mx[n + 16 + k, i, j]
        Mx[n + 16 + k, i, j] = complex(bad[(k + 1) % 3], z.imag) if part == 0 else complex(z.real, bad[(k + 1) % 3])
    Vx[n + 32], Mx[n + 33] = bad[3], bad[3]
    order = rng.permutation(2 * n)
    (g1, st1), _ = both(ctx, "flagged", Vx[order], Mx[order], np.tile(a1, 2)[order], np.tile(a2, 2)[order], 6,
                        slot=np.tile(sl, 2)[order], T=3, wt=wx[order], niter=6)
    assert st1[5] == n and np.array_equal(st1[[0, 4, 6, 7]], st0[[0, 4, 6, 7]])
    assert np.abs(g1 - g0).max() <= TOL * np.abs(g0).max() and np.isfinite(st1).all()
    assert abs(st1[2] - st0[2]) <= 1e-9 * st0[2] and abs(st1[3] - st0[3]) <= 1e-9 * st0[3]


# ---- chunking --------------------------------------------------------------------------------------------------------------
def stream(rng, n, A, T, order="time"):
    a1 = rng.integers(0, A, n)
    a2 = (a1 + rng.integers(1, A, n)) % A
    sl = rng.integers(0, T, n)
    if order == "time":
        sl = np.sort(sl)
    M = mats(rng, n)
    Gt = 0.2 * mats(rng, T, A) + np.eye(2)
    V = J.mm(J.mm(Gt[sl, a1], M), J.herm(Gt[sl, a2])) + 0.05 * mats(rng, n)
    return a1, a2, sl, V, M, rng.uniform(0.5, 2, n)


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_around_one_chunk(ctx, n):
    a1, a2, sl, V, M, w = stream(np.random.default_rng(n), n, 8, 3)
    both(ctx, f"n={n}", V, M, a1, a2, 8, slot=sl, T=3, wt=w, niter=3, forms=("dev",))


def test_interval_change_on_a_chunk_boundary_and_inside_a_chunk(ctx):
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
    """More chunks than the launch has work-groups: a work-group then takes a contiguous range of several chunks - the only
    size at which that path runs.  At the LDS limit a CU holds ONE work-group (of 1024 threads), so the stream needs only a
    chunk more than the device has CUs; one iteration keeps the numpy reference at a few seconds."""
    import gridhip
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    A = gridhip.jonescal_lds_antennas()
    n = (ncu + 1) * CHUNK + 5
    a1, a2, sl, V, M, w = stream(np.random.default_rng(11), n, A, 3)
    both(ctx, f"n={n}", V, M, a1, a2, A, slot=sl, T=3, wt=w, niter=1, forms=("dev",))


# ---- the LDS table's edges and the limit on A * T ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["a quarter", "half", "limit - 1", "limit", "limit + 1"])
def test_lds_table_edges(ctx, where):
    """The table of one interval takes 160 B per antenna: work-groups of 256 threads up to a quarter of the CU's LDS, of 512
    up to half, of 1024 at the limit; one antenna more and the sums go to global memory."""
    import gridhip
    lim = gridhip.jonescal_lds_antennas()
    A = {"a quarter": 255, "half": 256, "limit - 1": lim - 1, "limit": lim, "limit + 1": lim + 1}[where]
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
    g = torch.full((T, A + 1, 2, 2), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    from gridhip import GridHipError, _lib
    with pytest.raises(GridHipError) as ei:
        ctx.jonescal(dev(V), dev(M), dev(a1), dev(a2), A + 1, slot=dev(sl), nslots=T, gains=g)
    assert ei.value.code == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((g == 7 + 7j).all())
    with pytest.raises(GridHipError) as ei:
        ctx.apply_jones(g, dev(V), dev(a1), dev(a2), slot=dev(sl))
    assert ei.value.code == _lib.EUNSUPPORTED


# ---- the stop on the device ------------------------------------------------------------------------------------------------
def test_stop_on_the_device(ctx):
    rng = np.random.default_rng(139)
    a1, a2, sl, V, M, _ = polarised(rng, 7, 3, noise=0.02)
    w = rng.uniform(0.5, 2, len(a1))
    hist = []
    J.jonescal(V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=40, tol=0.0, history=hist)
    # rel falls in two interleaved sequences (averaged and plain iterations): a tol between iteration k's and the least
    # before it is first reached at k, and rounding (1e-15 of rel) cannot move that
    k = 1 + max(i for i in range(20, 40) if hist[i] < min(hist[:i]) / 1.2)
    tol = float(np.sqrt(hist[k - 1] * min(hist[:k - 1])))
    gr, sr = J.jonescal(V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=100, tol=tol)
    assert sr[0] == k and hist[k - 1] <= tol / 1.09 and min(hist[:k - 1]) >= 1.09 * tol
    g, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=100, tol=tol)
    agree("stopped", g, st, gr, sr)
    assert st[0] == k
    # exactly k iterations without a stop rule give the same gains: the 100 - k later launches changed nothing
    g2, st2 = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, wt=w, niter=k, tol=0.0)
    assert st2[0] == k and np.abs(g2 - g).max() <= TOL * np.abs(g).max() and abs(st2[1] - st[1]) <= 1e-9


def test_warm_start_reproduces_a_split_solve(ctx):
    rng = np.random.default_rng(14)
    a1, a2, sl, V, M, _ = polarised(rng, 6, 2, noise=0.05)
    w = rng.uniform(0.5, 2, len(a1))
    k = 4  # even: the second half then averages on the same iterations as the whole
    whole, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=2 * k, refant=-1)
    half, _ = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1)
    rest, st = solve(ctx, V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, refant=-1, gains=half)
    assert st[0] == k and np.abs(rest - whole).max() <= TOL * np.abs(whole).max()
    both(ctx, "warm", V, M, a1, a2, 6, slot=sl, T=2, wt=w, niter=k, gains=half)


# ---- recovery --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_noise_free_data_are_recovered(ctx, mode):
    """G_p M G_q^H is compared with V, never G with the truth: the gauge differs."""
    rng = np.random.default_rng(40 + mode)
    a1, a2, sl, V, M, _ = polarised(rng, 7, 3, diagonal=mode == 1)
    gr, sr = J.jonescal(V, M, a1, a2, 7, slot=sl, T=3, mode=mode, niter=300, tol=1e-13)
    assert sr[2] <= 1e-14 * sr[3] and sr[0] < 300  # the reference gets there on this very case
    g, st = solve(ctx, V, M, a1, a2, 7, slot=sl, T=3, mode=mode, niter=300, tol=1e-13)
    print(f"mode {mode}: {st[0]:.0f} iterations (reference {sr[0]:.0f}), chi2 / chi2_0 = {st[2] / st[3]:.2e}")
    assert st[2] <= 1e-10 * st[3] and st[7] == 0
    assert np.abs(J.mm(J.mm(g[sl, a1], M), J.herm(g[sl, a2])) - V).max() <= 1e-8 * np.abs(V).max()


# ---- apply -----------------------------------------------------------------------------------------------------------------
def jones(rng, *shape):
    """Jones matrices of condition number <= 10: U diag(s1, s2) W^H with s1 / s2 in [1, 10]"""
    q1, q2 = np.linalg.qr(mats(rng, *shape))[0], np.linalg.qr(mats(rng, *shape))[0]
    s = np.zeros(shape + (2, 2))
    s[..., 1, 1] = rng.uniform(0.3, 1.0, shape)
    s[..., 0, 0] = s[..., 1, 1] * rng.uniform(1, 10, shape)
    return q1 @ s @ np.conj(np.swapaxes(q2, -1, -2))


def apply_agrees(what, vo, wo, vr, wr):
    scale = np.abs(vr).reshape(len(vr), 4).max(axis=1, initial=0.0)[:, None, None]
    fin = np.isfinite(scale[:, 0, 0])
    err = (np.abs(vo - vr)[fin] / np.where(scale[fin] > 0, scale[fin], 1.0)).max(initial=0.0)
    print(f"{what}: {err:.2e}")
    assert vo.shape == vr.shape and err <= 1e-13, what
    assert np.allclose(wo, wr, rtol=1e-14, atol=0, equal_nan=True), what


def test_apply_both_directions_in_place_and_unusable_gains(ctx):
    import torch
    rng = np.random.default_rng(15)
    n, A, T = CHUNK + 33, 6, 3
    a1, a2, sl, V, M, w = stream(rng, n, A, T)
    a1[:6], a2[:6], sl[:6] = [-1, A, 0, 0, 1, 1], [0, 1, -1, A, 2, 1], [0, 0, 0, 0, T, 0]  # out of range; an autocorrelation
    g = jones(rng, T, A)
    g[1, 2] = [[1, 2], [2, 4]]                   # singular: det = 0 exactly
    g[2, 3] = np.eye(2) * 1e-90                  # |det|^2 = 1e-360 underflows
    g[0, 4] = np.eye(2) * 1e90                   # |det|^2 = 1e360 overflows
    g[2, 5, 0, 1] = np.nan
    w[7] = 0.0
    for inverse in (True, False):
        vr, wr = J.apply_jones(g, V, a1, a2, slot=sl, wt=w, inverse_=inverse)
        for form in ("host", "dev"):
            if form == "host":
                vo, wo = ctx.apply_jones(g, V, a1, a2, slot=sl, weights=w, inverse=inverse)
            else:
                vo, wo = (host(x) for x in ctx.apply_jones(dev(g), dev(V), dev(a1), dev(a2), slot=dev(sl), weights=dev(w),
                                                           inverse=inverse))
            fin = np.isfinite(vr).all(axis=(1, 2))
            assert np.array_equal(fin, np.isfinite(vo).all(axis=(1, 2)))
            apply_agrees(f"inverse={inverse} [{form}]", vo[fin], wo[fin], vr[fin], wr[fin])
            if inverse:
                unusable = ~((a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A) & (sl >= 0) & (sl < T))
                ok = ~unusable
                badg = np.zeros((T, A), dtype=bool)
                badg[1, 2] = badg[2, 3] = badg[0, 4] = badg[2, 5] = True
                unusable[ok] = badg[sl[ok], a1[ok]] | badg[sl[ok], a2[ok]]
                assert unusable.sum() > 20 and np.array_equal(vo[unusable], V[unusable])
                assert np.all(wo[unusable] == 0.0) and not np.signbit(wo[unusable]).any() and np.all(wo[~unusable & (w > 0)] > 0)
    # without weights: ones; in place; and correcting what was corrupted gives the input back
    good = jones(rng, T, A)
    dv, dw = dev(V), dev(w)
    v0, _ = ctx.apply_jones(dev(good), dv, dev(a1), dev(a2), slot=dev(sl), inverse=False, out=dv)
    assert v0 is dv
    vb, wb = ctx.apply_jones(dev(good), dv, dev(a1), dev(a2), slot=dev(sl), weights=dw, out=dv, weights_out=dw)
    assert vb is dv and wb is dw
    torch.cuda.synchronize()
    # (two applications, each within 1e-13 of its output scaled by the conditioning: <= 10 per matrix, four matrices)
    assert np.abs(host(dv) - V).max() <= 1e-11 * np.abs(V).max()
    _, wr = J.apply_jones(good, V, a1, a2, slot=sl, wt=w)
    assert np.allclose(host(dw), wr, rtol=1e-14, atol=0)
    _, w1 = ctx.apply_jones(good, V, a1, a2, slot=sl)
    assert np.allclose(w1, J.apply_jones(good, V, a1, a2, slot=sl)[1], rtol=1e-14, atol=0)


def test_scalar_jones_matrices_are_apply_gains_on_each_correlation(ctx):
    rng = np.random.default_rng(16)
    n, A, T = 500, 5, 2
    a1, a2, sl, V, _, w = stream(rng, n, A, T)
    g = (1 + 0.3 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-2, 2, (T, A)))
    G = np.ascontiguousarray(g[..., None, None] * np.eye(2))
    for inverse in (True, False):
        vj, wj = ctx.apply_jones(G, V, a1, a2, slot=sl, weights=w, inverse=inverse)
        for i in (0, 1):
            for j in (0, 1):
                vs, ws = ctx.apply_gains(g, np.ascontiguousarray(V[:, i, j]), a1, a2, slot=sl, weights=w, inverse=inverse)
                ev, ew = np.abs(vj[:, i, j] - vs).max() / np.abs(vs).max(), (np.abs(wj - ws) / ws).max()
                print(f"inverse={inverse} correlation {i}{j}: vis {ev:.2e} of the largest, weights {ew:.2e} relative")
                assert ev <= 1e-15 and ew <= 1e-15


@pytest.mark.parametrize("n", [0, 1, 257])  # none, one, one work-group and one
def test_apply_host_and_device_forms_give_the_same_bits(ctx, n):
    """Every staging branch of gridhip_apply_jones: slot, wt_in and wt_out present and null, out of place and in place."""
    rng = np.random.default_rng(300 + n)
    A, T = 3, 2
    a1, a2, sl, V, _, w = stream(rng, n, A, T)
    g = jones(rng, T, A)
    for slot in (sl, None):
        gg = g if slot is not None else g[:1].copy()
        for wt in (w, None):
            for want_wo in (True, False):
                for in_place in (False, True):
                    for inverse in (1, 0):
                        vin = V.copy()
                        vout = vin if in_place else np.full((n, 2, 2), 7 - 7j)
                        wi = None if wt is None else wt.copy()
                        wo = None if not want_wo else wi if in_place and wi is not None else np.full(n, 7.0)
                        hst, dvc = both_forms(ctx, "apply_jones", [n, A, len(gg), a1, a2, slot, gg, inverse, vin, wi, vout, wo])
                        what = (n, slot is not None, wt is not None, want_wo, in_place, inverse)
                        for k in hst:
                            assert hst[k].tobytes() == dvc[k].tobytes(), what
                        for x in (a1, a2, gg) + (() if in_place else (vin,)):
                            assert hst[id(x)].tobytes() == x.tobytes(), what  # inputs as they were
                        vr, wr = J.apply_jones(gg, V, a1, a2, slot=slot, wt=wt, inverse_=bool(inverse))
                        apply_agrees(str(what), hst[id(vout)], wr if wo is None else hst[id(wo)], vr, wr)


# ---- stokes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257, CHUNK + 3])
def test_stokes_is_numpy_to_the_bit(ctx, n):
    rng = np.random.default_rng(500 + n)
    V = mats(rng, n)
    if n > 1:
        V[0] = 0.0
        V[1] = [[-0.0, -1], [1, complex(0.0, -0.0)]]  # (signed zeros; a NaN's sign and payload are no part of the contract)
    for basis, name in ((0, "linear"), (1, "circular")):
        full = J.stokes(V, basis)
        for which in range(1, 16):
            letters = "".join(c for b, c in enumerate("IQUV") if which >> b & 1)
            fill = np.full((4, n), 7 - 7j)
            want = J.stokes(V, basis, which, out=fill)
            got_h = ctx.stokes(V, basis=name, which=letters, out=fill.copy())
            got_d = host(ctx.stokes(dev(V), basis=name, which=letters, out=dev(fill)))
            assert got_h.tobytes() == want.tobytes() and got_d.tobytes() == want.tobytes(), (name, letters)
        assert ctx.stokes(V, basis=name).tobytes() == full.tobytes()  # a new block: all four rows written
        S = mats(rng, 1)[0].reshape(4, 1) * np.ones((1, n)) + (rng.normal(size=(4, n)) if n else 0)
        want = J.stokes_inverse(S, basis)
        assert ctx.stokes(S, basis=name, inverse=True).tobytes() == want.tobytes()
        assert host(ctx.stokes(dev(S), basis=name, inverse=True)).tobytes() == want.tobytes()
        # short mantissas: the round trip is the identity to the bit
        S8 = (rng.integers(-64, 64, (4, n)) + 1j * rng.integers(-64, 64, (4, n))) / 8
        back = ctx.stokes(ctx.stokes(dev(S8), basis=name, inverse=True), basis=name)
        assert host(back).tobytes() == S8.astype(c128).tobytes()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header, through the C ABI on device memory: GRIDHIP_EINVAL and the outputs as they were given."""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    n, A, T = 5, 3, 2
    full = lambda shape, val, dt=torch.complex128: torch.full(shape, val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(a1=to_dev(np.array([0, 0, 1, 0, 1], dtype=i64)), a2=to_dev(np.array([1, 2, 2, 1, 2], dtype=i64)),
             sl=to_dev(np.array([0, 0, 0, 1, 1], dtype=i64)), v=full((2 * n, 2, 2), 2 + 1j), m=full((n, 2, 2), 1 - 1j),
             w=full((n,), 1.5, torch.float64), g=full((T * A + 1, 2, 2), 7 + 7j), st=full((8,), 9.0, torch.float64),
             o=full((n, 2, 2), 3 + 3j), wo=full((n,), 4.0, torch.float64), sk=full((4, n), 5 - 5j))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    h = ctx._h

    def jc(n=n, A=A, T=T, a1=p["a1"], a2=p["a2"], sl=p["sl"], v=p["v"], m=p["m"], w=p["w"], mode=0, ref=0, warm=0,
           niter=3, tol=0.0, g=p["g"], st=p["st"]):
        return lib.gridhip_jonescal_dev(h, n, A, T, a1, a2, sl, v, m, w, mode, ref, warm, niter, tol, g, st)

    def ap(n=n, A=A, T=T, a1=p["a1"], a2=p["a2"], sl=p["sl"], g=p["g"], inv=1, v=p["v"], w=p["w"], o=p["o"], wo=p["wo"]):
        return lib.gridhip_apply_jones_dev(h, n, A, T, a1, a2, sl, g, inv, v, w, o, wo)

    def sk(n=n, basis=0, which=15, inv=0, v=p["v"], s=p["sk"]):
        return lib.gridhip_stokes_dev(h, n, basis, which, inv, v, s)

    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    bad = [jc(n=-1), jc(A=1), jc(T=0), jc(sl=None), jc(a1=None), jc(a2=None), jc(v=None), jc(m=None), jc(g=None),
           jc(niter=-1), jc(tol=-1.0), jc(tol=float("nan")), jc(mode=3), jc(mode=-1), jc(ref=A), jc(g=p["v"]), jc(g=p["m"]),
           jc(g=p["w"]), jc(g=p["a1"]), jc(g=p["a2"]), jc(g=p["sl"]), jc(g=at("v", 64 * n - 8), v=p["v"]),
           ap(n=-1), ap(A=1), ap(T=0), ap(sl=None), ap(a1=None), ap(a2=None), ap(g=None), ap(v=None), ap(o=None), ap(inv=2),
           ap(inv=-1), ap(o=p["g"]), ap(wo=p["g"]), ap(o=p["a1"]), ap(wo=p["sl"]), ap(o=at("v", 64)), ap(wo=at("w", 8)),
           ap(o=p["w"]), ap(wo=p["o"]),
           sk(n=-1), sk(basis=2), sk(basis=-1), sk(which=0), sk(which=16), sk(inv=2), sk(inv=-1), sk(inv=1, which=7),
           sk(v=None), sk(s=None), sk(s=p["v"]), sk(s=at("v", 64 * n - 16)), sk(inv=1, s=at("v", 16), v=p["v"])]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), bad
    assert jc(A=1 << 11, T=(1 << 10) + 1) == _lib.EUNSUPPORTED and ap(A=(1 << 21) + 1, T=1, sl=None) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    for key, val in (("g", 7 + 7j), ("st", 9.0), ("o", 3 + 3j), ("wo", 4.0), ("v", 2 + 1j), ("w", 1.5), ("sk", 5 - 5j),
                     ("m", 1 - 1j)):
        assert bool((t[key] == val).all()), key
    # and the valid corners next to them: T == 1 without slot, no weights, no stats, no rotation, wt_out NULL, n == 0
    assert jc(T=1, sl=None, w=None, st=None, ref=-1, mode=2) == 0 and ap(T=1, sl=None, w=None, wo=None) == 0
    assert jc(n=0, a1=None, a2=None, sl=None, v=None, m=None, w=None, T=1) == 0 and ap(n=0, v=None, o=None, a1=None, a2=None) == 0
    assert sk(n=0, v=None, s=None) == 0 and sk(which=4) == 0 and sk(inv=1, v=p["o"]) == 0
    ctx.synchronize()
    assert bool((t["sk"][[0, 1, 3]] == 5 - 5j).all()) and not bool((t["sk"][2] == 5 - 5j).any())


# ---- a graph, and the whole chain ------------------------------------------------------------------------------------------
def test_a_captured_chain_replays_to_the_eager_result(ctx):
    import torch
    rng = np.random.default_rng(21)
    a1, a2, sl, V, M, _ = polarised(rng, 6, 2, noise=0.02)
    n = len(a1)
    dV, dM, d1, d2, dsl, dw = dev(V), dev(M), dev(a1), dev(a2), dev(sl), dev(rng.uniform(0.5, 2, n))
    kw = dict(slot=dsl, nslots=2, weights=dw, niter=40, tol=0.0)
    g = torch.empty((2, 6, 2, 2), dtype=torch.complex128, device="cuda:0")
    out, wout, blk = torch.empty_like(dV), torch.empty_like(dw), torch.empty((4, n), dtype=torch.complex128, device="cuda:0")

    def chain():
        # (a warm start from the identity written by a kernel of torch's: the same gains array on every replay)
        g.zero_()
        g[..., 0, 0] = 1
        g[..., 1, 1] = 1
        _, stats = ctx.jonescal(dV, dM, d1, d2, 6, gains=g, **kw)
        ctx.apply_jones(g, dV, d1, d2, slot=dsl, weights=dw, out=out, weights_out=wout)
        ctx.stokes(out, out=blk)
        return stats
    stats = chain()
    torch.cuda.synchronize()
    eager = [host(x).copy() for x in (g, out, wout, blk, stats)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        stats = chain()
    torch.cuda.synchronize()
    for _ in range(2):
        g.fill_(7.0), out.fill_(7.0), wout.fill_(7.0), blk.fill_(7.0), stats.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        G, O, W, B, S = (host(x) for x in (g, out, wout, blk, stats))
        assert np.abs(G - eager[0]).max() <= TOL * np.abs(eager[0]).max()
        assert np.abs(O - eager[1]).max() <= 1e-9 * np.abs(eager[1]).max() and np.allclose(W, eager[2], rtol=1e-9, atol=0)
        assert np.abs(B - eager[3]).max() <= 1e-9 * np.abs(eager[3]).max()
        assert np.array_equal(S[[0, 4, 5, 6, 7]], eager[4][[0, 4, 5, 6, 7]]) and S[0] == 40


def test_stokes_predictions_to_calibrated_stokes_streams(ctx):
    """Four Stokes point-source streams -> stokes(inverse) -> corrupted with known Jones matrices -> jonescal -> apply_jones
    -> stokes: the I stream is the uncorrupted one again.  Three sources of different polarisation: the model then varies
    from sample to sample and fixes the gauge up to the common phase."""
    rng = np.random.default_rng(22)
    A, T = 7, 2
    p, q = np.triu_indices(A, 1)
    a1, a2, sl = np.tile(p, 3 * T), np.tile(q, 3 * T), np.repeat(np.arange(T), 3 * len(p))
    n = len(a1)
    u, v = rng.uniform(-500, 500, n), rng.uniform(-500, 500, n)
    lm = np.array([[0.001, -0.002], [-0.003, 0.0015], [0.002, 0.0025]])
    iquv = np.array([[3.0, 2.0, 0.5, -0.4], [2.0, -1.2, 1.0, 0.6], [1.5, 0.3, -1.0, 0.9]])  # I, Q, U, V per source
    phase = np.exp(-2j * np.pi * (np.outer(lm[:, 0], u) + np.outer(lm[:, 1], v)))            # [source][n]
    S = np.ascontiguousarray(np.einsum("sk,sn->kn", iquv, phase))                             # four streams [4][n]
    dS, d1, d2, dsl = dev(S), dev(a1), dev(a2), dev(sl)
    model = ctx.stokes(dS, inverse=True)
    Gt = dev(0.2 * mats(rng, T, A) + np.eye(2))
    vis = ctx.apply_jones(Gt, model, d1, d2, slot=dsl, inverse=False)[0]
    assert float((vis - model).abs().max()) > 0.1
    g, st = ctx.jonescal(vis, model, d1, d2, A, slot=dsl, nslots=T, niter=300, tol=1e-13)
    cal, wcal = ctx.apply_jones(g, vis, d1, d2, slot=dsl)
    back = host(ctx.stokes(cal))
    st = host(st)
    err = np.abs(back[0] - S[0]).max() / np.abs(S[0]).max()
    print(f"{st[0]:.0f} iterations, chi2 / chi2_0 = {st[2] / st[3]:.2e}, I stream {err:.2e}, all four "
          f"{np.abs(back - S).max() / np.abs(S).max():.2e}")
    assert st[2] <= 1e-10 * st[3] and st[7] == 0
    assert err <= 1e-8
    assert bool((wcal > 0).all())
