"""GPU parity for the operations either side of the gridder (csrc/image_ops.hip, csrc/fft.hip) at their edge shapes:
the branches and sizes that tests/test_gpu_imaging.py's one random draw per operation never reaches.  Every case
compares with the C oracle, and with the numpy oracle too where it has the operation.

Tolerances are the project's own: exact equality for integer outputs, mirror_uvw and make_grid_hermitian, 1e-15
relative for doweight, TOL = 1e-10 relative for anything behind a transform, 1e-12 for an imager against itself."""
import ctypes as C

import numpy as np
import pytest

from image_ops_cases import BELOW_HALF, WKERNEL_REFUSED, WSTEPS, tie_vector
from oracle import gridref_np as P

pytestmark = pytest.mark.gpu
TOL = 1e-10


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def bits(a):
    """the bit patterns of a float64 or complex128 array: -0.0 and NaN payloads count"""
    a = np.ascontiguousarray(a)
    return (a.view(np.float64) if a.dtype == np.complex128 else a).view(np.uint64)


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- the w-bin rule -------------------------------------------------------------------------------------------------------
def wave_positions(n):
    """index 0, index n - 1, the last element of the last full wave of 64, and one inside the partial last wave"""
    pos = [0, n - 1]
    if n >= 64:
        pos.append((n // 64) * 64 - 1)
    if n % 64:
        pos.append((n // 64) * 64 + (n % 64) // 2)
    return list(dict.fromkeys(pos))


@pytest.mark.parametrize("wstep", WSTEPS)
def test_wbins_ties_extremes_and_stride(ctx, oracle, wstep):
    """wround_kernel's grid-stride loop and cross-wave reduction: the grid is capped at 4 work-groups per CU, so 300 001
    values make the loop stride (65 and 257 leave a partial last wave, 63 has no full one); the unique minimum and
    the unique maximum take turns at index 0, index n - 1, the last lane of a full wave and inside the partial last
    wave, where a reduction that drops a lane, a wave or the tail loses them.  The values hold every tie
    w / wstep = k + 0.5 for both signs, +-0.0, the doubles next to each tie and the largest double below wstep / 2."""
    rng = np.random.default_rng(100 + wstep)
    ties = tie_vector(wstep)
    lo, hi = -20.25 * wstep, 23.25 * wstep  # round to -20 and 23: 44 planes
    for x in (ties[0], ties[9], -0.0, ties[18], 0.5 * wstep, BELOW_HALF * wstep):
        got, ref = ctx.wbins(np.array([x]), wstep), oracle.wbins(np.array([x]), wstep)
        assert list(got[0]) == list(ref[0]) == [0] and got[1:] == ref[1:] and got[2] == 1, x
    for n in (63, 64, 65, 257, 300_001):
        base = rng.permutation(np.concatenate([ties, rng.uniform(-4.0 * wstep, 4.0 * wstep, max(n - len(ties), 0))]))[:n]
        pos = wave_positions(n)
        for i, imin in enumerate(pos):
            imax = pos[(i + 1) % len(pos)]
            w = base.copy()
            w[imin], w[imax] = lo, hi
            wb, mn, npl = ctx.wbins(w, wstep)
            rb, rmn, rnpl = oracle.wbins(w, wstep)
            assert (rmn, rnpl) == (-20 * wstep, 44) and rb[imin] == 0 and rb[imax] == 43
            assert (mn, npl) == (rmn, rnpl), (n, imin, imax)
            assert wb.dtype == np.int64 and np.array_equal(wb, rb), (n, imin, imax)
            pb, pmn, pnpl = P.wbins(w, wstep)
            assert np.array_equal(pb, rb) and (pmn, pnpl) == (rmn, rnpl)
    wb, mn, npl = ctx.wbins(np.empty(0), wstep)
    assert len(wb) == 0 and (mn, npl) == (0, 0)


# ---- findClosest ------------------------------------------------------------------------------------------------------------
def plane_lists():
    rng = np.random.default_rng(51)
    few = rng.uniform(-50.0, 50.0, 900)
    return [np.array([3.0]), np.array([0.0, 1.0]), np.array([0.0, 1.0, 2.0]),
            np.array([0.0, 1.0, 1.0, 2.0, 4.0, 4.0, 4.0, 7.0]), np.sort(rng.uniform(0.0, 100.0, 129)),
            np.sort(np.concatenate([few, rng.choice(few, 100, replace=False)]))]


@pytest.mark.parametrize("which", range(6))
def test_find_closest_degenerate_inputs(ctx, oracle, which):
    """closest_index's degenerate inputs: nws of 1 and 2, repeated plane values (1 000 planes, 100 of them duplicates),
    x exactly on a plane, x exactly half-way between two planes and the doubles either side of both, x outside the
    range, +-inf and NaN x (every comparison false: whatever index the oracles return for it, the kernel returns)."""
    ws = plane_lists()[which]
    assert which != 5 or (len(ws) == 1000 and len(np.unique(ws)) == 900)
    mid = (ws[:-1] + ws[1:]) / 2.0
    exact = np.concatenate([ws, mid])
    x = np.concatenate([exact, np.nextafter(exact, np.inf), np.nextafter(exact, -np.inf),
                        [ws[0] - 1.0, ws[0] - 1e300, ws[-1] + 1.0, ws[-1] + 1e300, np.inf, -np.inf, np.nan]])
    got = ctx.findClosest(ws, x)
    ref = np.array([oracle.find_closest(ws, xi) for xi in x])
    assert got.dtype == np.int64 and np.array_equal(got, ref)
    assert np.array_equal(ref, np.array([P.find_closest(ws, xi) for xi in x]))
    assert 0 <= ref.min() and ref.max() <= len(ws) - 1


# ---- mirror_uvw -------------------------------------------------------------------------------------------------------------
SPECIAL_V = [0.0, -0.0, -5e-324, np.nan, np.inf, -np.inf]


def check_mirror(ctx, oracle, u, v, w, vis):
    (mu, mv, mw), mvis = ctx.mirror_uvw((u, v, w), vis)
    for ref in (oracle.mirror_uvw(u, v, w, vis), P.mirror_uvw(u, v, w, vis)):
        for a, b in zip((mu, mv, mw, mvis), ref):
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_001])
def test_mirror_uvw_signed_zeros_denormals_nan_inf(ctx, oracle, n):
    """mirror_kernel's one comparison, v < 0, on the values where it can go wrong: 0.0 and -0.0 (not mirrored), the
    smallest negative denormal (mirrored: a flush to zero would not), NaN (not mirrored, payload kept) and +-inf, among
    random values; n around one work-group of 256 and above one grid of them.  Bit-identical to both oracles."""
    rng = np.random.default_rng(60 + n)
    if n == 1:
        for s in SPECIAL_V + [-1.5, 2.5]:
            check_mirror(ctx, oracle, np.array([0.0]), np.array([s]), np.array([-3.0]), np.array([1.0 + 0.0j]))
        return
    u, v, w = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    at = np.unique(np.concatenate([[0, 1, n - 1, n - 2, 255 % n, 256 % n], rng.choice(n, 48, replace=False)]))
    v[at] = np.resize(SPECIAL_V, len(at))
    u[at[::2]], vis[at[::3]] = 0.0, 0.0  # (mirrored zeros become -0.0)
    assert (v < 0).sum() > n // 3 and np.isnan(v).sum() >= 8
    check_mirror(ctx, oracle, u, v, w, vis)


# ---- doweight ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 128, 129])
def test_doweight_outside_boundaries_crowded_cell_nan(ctx, oracle, N):
    """weight_cell returning -1, under doweight itself: points spread to +-0.7 of the field and a few to +-0.9 (a share outside the
    grid on each of its four sides), points exactly on cell boundaries (halfN + p * N + 0.5 an integer) and at the grid's first
    and last cell, 60 000 points in one cell, and NaN u, NaN v and both.  A row outside the grid or with a NaN
    coordinate comes back bit-identical ("the weight stays 1") and changes no other row's count."""
    theta, lam = 0.25, 4 * N
    assert ctx.image_size(theta, lam) == N == P.haskell_round(theta * lam)
    rng = np.random.default_rng(70 + N)
    half = N // 2
    # (the cells cover [-(half + 0.5) / N, (N - half - 0.5) / N): down to -0.75 for N = 2, which +-0.7 does not leave -
    # 600 further points spread to +-0.9 put a share outside on that side too)
    ua, va = (np.concatenate([rng.uniform(-0.7, 0.7, 3000), rng.uniform(-0.9, 0.9, 600)]) * lam for _ in range(2))
    # u / lam * N = j - 0.5 - half for j = 0 .. N (u is an exact integer), then the first and the last cell's centres
    edge = np.concatenate([4.0 * np.arange(N + 1) - 2.0 - 4.0 * half, [-4.0 * half, 4.0 * (N - 1 - half)]])
    ub = np.concatenate([edge, edge, edge])
    vb = np.concatenate([edge, np.roll(edge, 1), np.roll(edge, 3)])
    cy, cx = N // 3, N // 2
    uc = 4.0 * (cx - half + rng.uniform(-0.4, 0.4, 60_000))
    vc = 4.0 * (cy - half + rng.uniform(-0.4, 0.4, 60_000))
    nan = np.nan
    u = np.concatenate([ua, ub, uc, [nan, 1.0, nan]])
    v = np.concatenate([va, vb, vc, [1.0, nan, nan]])
    n = len(u)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    pu, pv = u / np.float64(lam), v / np.float64(lam)
    fin = np.isfinite(pu) & np.isfinite(pv)
    x, y = np.full(n, -1), np.full(n, -1)
    x[fin], y[fin] = oracle.frac_coord(N, 1, pu[fin])[0], oracle.frac_coord(N, 1, pv[fin])[0]
    keep = fin & (x >= 0) & (x < N) & (y >= 0) & (y < N)
    a = slice(0, 3600)
    assert min((x[a] < 0).sum(), (x[a] >= N).sum(), (y[a] < 0).sum(), (y[a] >= N).sum()) > 20
    b = slice(3600, 3600 + len(ub))
    xe = half + pu[b] * N + 0.5
    on = xe == np.floor(xe)
    assert on.sum() >= 3 and (N & (N - 1) or on[:N + 1].all())  # (every boundary where N is a power of two)
    assert 0 in x[b] and N - 1 in x[b] and N in x[b] and 0 in y[b] and N - 1 in y[b]
    assert ((x == cx) & (y == cy)).sum() >= 60_000 and (~keep).sum() > 1000
    got = ctx.doweight(theta, lam, (u, v, None), vis)
    assert rel(got[fin], oracle.doweight(N, pu[fin], pv[fin], vis[fin])) < 1e-15
    assert rel(got[fin], P.doweight(N, pu[fin], pv[fin], vis[fin])) < 1e-15
    assert np.array_equal(bits(got[~keep]), bits(vis[~keep]))
    ratio = np.abs(got[keep]) / np.abs(vis[keep])  # 1 / count
    assert ratio.max() <= 1.0 + 1e-12 and ratio.min() < 1.0001 / 60_000
    alone = ctx.doweight(theta, lam, (u[keep], v[keep], None), vis[keep])
    assert np.array_equal(bits(alone), bits(got[keep]))


# ---- make_grid_hermitian ------------------------------------------------------------------------------------------------------
def same_values(a, b):
    """equal, NaN where the other has NaN (inf - inf), and zeros of the same sign"""
    a, b = a.view(np.float64), b.view(np.float64)
    ok = ~np.isnan(b)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[ok], b[ok])
            and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok])))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 64, 65, 255])
def test_make_grid_hermitian_small_odd_even_and_special_values(ctx, oracle, N):
    """hermitian_kernel's two branches at the sizes where its index arithmetic degenerates (1, 2, 3), at even and odd
    sizes below and above one work-group, on random input and on input with -0.0 and +-inf entries: an even grid's
    first row and column get 0 :+ 0 added (an imaginary -0.0 becomes +0.0), every other cell the mirrored conjugate."""
    rng = np.random.default_rng(80 + N)
    g = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    ref = oracle.make_grid_hermitian(g)
    assert np.array_equal(ctx.make_grid_hermitian(g), ref) and np.array_equal(P.make_grid_hermitian(g), ref)
    s = g.copy()
    flat = s.reshape(-1)
    flat[::3] = complex(-0.0, -0.0)
    flat[1::7] = complex(np.inf, -1.0)
    flat[2::11] = complex(2.0, -np.inf)
    flat[0] = complex(-0.0, -0.0)
    if N >= 4:  # inf meets -inf: the mirror of (1, 1) is (N - 1, N - 1) on an even grid, (N - 2, N - 2) on an odd one
        s[1, 1], s[N - 1, N - 1], s[N - 2, N - 2] = complex(np.inf, 1.0), complex(-np.inf, 1.0), complex(-np.inf, 1.0)
    ref = oracle.make_grid_hermitian(s)
    assert same_values(ctx.make_grid_hermitian(s), ref)
    assert N < 4 or (np.isnan(ref[1, 1].real) and np.isinf(ref.view(np.float64)).any())


# ---- the centred transform and the context's four plan slots -------------------------------------------------------------------
def test_centred_fft_across_plan_cache_evictions(ctx, oracle):
    """The plan cache in fft_plan_for holds four sizes and evicts round-robin after a stream synchronisation: nine sizes
    (2 and 3, primes, powers of 3 and 5, even composites) are cycled forward and then backward, so every size is
    re-created after its eviction, and fft and ifft are compared each time.  Between steps the w-kernel generator takes
    a slot of its own (na = 99), and an imager made before the loop cycles: it owns its plan and must not notice."""
    import torch
    sizes = [2, 3, 64, 97, 100, 125, 127, 240, 243]
    rng = np.random.default_rng(90)
    case = {}
    for N in sizes:
        a = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
        refs = [(oracle.fft2_centered(a, inv), fn(a)) for inv, fn in ((False, P.fft_c), (True, P.ifft_c))]
        assert all(rel(c, p) < TOL for c, p in refs)
        case[N] = (a, refs)
    kref = oracle.w_kernel(0.1, 300.0, 33, 9, 3)
    theta, lam, n = 0.1, 490, 500  # N = 49
    u, v, w = (rng.uniform(-0.55, 0.55, n) * lam for _ in range(3))
    dvis = to_dev(rng.normal(size=n) + 1j * rng.normal(size=n))
    im = ctx.imager(theta, lam, tuple(to_dev(x) for x in (u, v, w)), ("simple",))
    first = im.cycle(dvis).cpu().numpy()
    vis_h = dvis.cpu().numpy()
    ref_img = P.do_imaging(theta, lam, u, v, w, vis_h, lambda th, la, uu, vv, ww, vs: P.grid(np.zeros((49, 49), complex),
                                                                                            uu / la, vv / la, vs))[0]
    assert rel(first, ref_img) < TOL
    for N in sizes + sizes[::-1]:
        a, refs = case[N]
        for got, (c, p) in zip((ctx.fft(a), ctx.ifft(a)), refs):
            assert rel(got, c) < TOL and rel(got, p) < TOL, N
        assert rel(ctx.w_kernel(0.1, 300.0, 33, 9, 3), kref) < TOL, N
        again = im.cycle(dvis).cpu().numpy()
        assert rel(again, first) < 1e-12, N
    torch.cuda.synchronize()
    assert ctx.get_option("errors") == 0
    im.close()


# ---- the w-kernel generator -----------------------------------------------------------------------------------------------------
W_KERNEL_SHAPES = [(32, 9, 1, 300.0),    # wkern_farfield_kernel's n == na branch (qpx == 1: no padding, no transposition), even
                   (33, 9, 1, 300.0),    # n == na, odd: the folded rolls differ, na / 2 against (na + 1) / 2
                   (33, 9, 3, 750.0),    # odd padded side na = npixFF * qpx = 99
                   (31, 8, 3, 750.0),    # na = 93 and an even npixKern
                   (32, 8, 2, 100.0),    # even npixKern, even na
                   (16, 15, 2, 50.0),
                   (16, 16, 1, 50.0),    # the whole far field is extracted
                   (17, 17, 1, 50.0),
                   (9, 9, 2, 10.0),      # na / 2 - qpx * (npixKern / 2) = 1 = qpx - 1: the last legal shape
                   (21, 7, 5, 2000.0),
                   (32, 1, 4, 100.0),
                   (32, 9, 2, 0.0),
                   (32, 9, 2, -400.0)]


@pytest.mark.parametrize("npixFF,S,Q,w", W_KERNEL_SHAPES)
def test_w_kernel_edge_shapes(ctx, oracle, npixFF, S, Q, w):
    """wkern_farfield_kernel's n == na branch (qpx == 1), odd padded sides na = npixFF * qpx (the two folded rolls then
    differ), even npixKern, supports of 1 and of the whole far field, w = 0 and w < 0, and the last shape the extraction
    can serve without reading before row 0."""
    assert (npixFF * Q) // 2 - Q * (S // 2) >= Q - 1
    got = ctx.w_kernel(0.1, w, npixFF, S, Q)
    ref = oracle.w_kernel(0.1, w, npixFF, S, Q)
    assert got.shape == (Q, Q, S, S) and np.abs(ref).max() > 0
    assert rel(got, ref) < TOL
    assert rel(got, P.w_kernel(0.1, w, npixFF, S, Q)) < TOL


def test_w_kernel_shapes_that_extract_outside_the_far_field_are_refused(ctx, oracle):
    """(npixFF, npixKern, qpx) with na / 2 - qpx * (npixKern / 2) < qpx - 1 - (8, 8, 2) and (16, 16, 2) - would make
    wkern_extract_kernel read before row 0 of the transform (it wrapped round silently): GRIDHIP_EINVAL with a message
    from gridhip_w_kernel and from every w_cache path, the output untouched, nothing counted in "errors" (that option
    counts the tile kernels' internal failures, not refusals), and the context as usable as before."""
    import gridhip
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    theta, lam, n = 0.05, 2560, 50
    rng = np.random.default_rng(95)
    u, v, w = (np.ascontiguousarray(rng.uniform(-500, 500, n)) for _ in range(3))
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(128, 128))
    du, dv, dw, dvis = (to_dev(x) for x in (u, v, w, vis))
    for nff, s, q in WKERNEL_REFUSED:
        out = np.full((q, q, s, s), 7 - 3j)
        assert lib.gridhip_w_kernel(h, 0.1, 50.0, nff, s, q, p(out)) == _lib.EINVAL
        assert "w-kernel shape" in lib.gridhip_last_error(h).decode()
        assert np.all(out == 7 - 3j)
        grid = np.full((128, 128), 7 - 3j)
        assert lib.gridhip_w_cache_imaging(h, 100, q, nff, s, theta, lam, n, p(u), p(v), p(w), 1, p(vis),
                                           p(grid)) == _lib.EINVAL
        assert "w-kernel shape" in lib.gridhip_last_error(h).decode() and np.all(grid == 7 - 3j)
        ko = dict(wstep=100, qpx=q, npixFF=nff, npixKern=s)
        calls = [lambda: ctx.w_kernel(0.1, 50.0, nff, s, q),
                 lambda: ctx.w_cache_imaging(ko, theta, lam, (u, v, w), None, vis),
                 lambda: ctx.w_cache_imaging(ko, theta, lam, (du, dv, dw), None, dvis),
                 lambda: ctx.do_imaging(theta, lam, (u, v, w), None, None, None, 1.0e8, vis, ("w_cache", ko)),
                 lambda: ctx.do_imaging(theta, lam, (du, dv, dw), None, None, None, 1.0e8, dvis, ("w_cache", ko)),
                 lambda: ctx.predict(theta, lam, (u, v, w), model, ("w_cache", ko)),
                 lambda: ctx.imager(theta, lam, (du, dv, dw), ("w_cache", ko))]
        for k, call in enumerate(calls):
            with pytest.raises(gridhip.GridHipError) as ei:
                call()
            assert ei.value.code == _lib.EINVAL, k
    assert ctx.get_option("errors") == 0
    assert rel(ctx.w_kernel(0.1, 10.0, 9, 9, 2), oracle.w_kernel(0.1, 10.0, 9, 9, 2)) < TOL


def test_w_cache_imaging_qpx1_and_odd_na_alternating(ctx):
    """w_cache_imaging, host and resident forms, with the generator's n == na branch (qpx = 1, npixFF = 32) and with an
    odd padded side (qpx = 3, npixFF = 33: na = 99), on an even and an odd grid (N = 128, 127).  The two kernel shapes
    alternate call by call: the table the context keeps (wk_cache) must not serve one shape's planes to the other."""
    import torch
    n = 1500
    rng = np.random.default_rng(96)
    kos = [dict(wstep=100, qpx=1, npixFF=32, npixKern=9), dict(wstep=100, qpx=3, npixFF=33, npixKern=9)]
    for lam, N in ((2560, 128), (2540, 127)):
        theta = 0.05
        assert ctx.image_size(theta, lam) == N
        u, v = rng.uniform(-0.53, 0.53, n) * lam, rng.uniform(-0.53, 0.53, n) * lam  # some fall outside the grid
        w = rng.uniform(-300, 300, n)
        vis = rng.normal(size=n) + 1j * rng.normal(size=n)
        refs = [P.w_cache_imaging(theta, lam, u, v, w, vis, ko["wstep"], ko["qpx"], ko["npixFF"], ko["npixKern"])
                for ko in kos]
        assert all(r[1].shape[0] == 7 for r in refs)  # (planes)
        d3, dvis = to_dev(np.stack([u, v, w], 1)), to_dev(vis)
        for resident in (False, True, False):
            for ko, (ref, _, _) in zip(kos, refs):
                if resident:
                    got = ctx.w_cache_imaging(ko, theta, lam, d3, None, dvis)
                    torch.cuda.synchronize()
                    got = got.cpu().numpy()
                else:
                    got = ctx.w_cache_imaging(ko, theta, lam, (u, v, w), None, vis)
                assert rel(got, ref) < TOL, (N, ko["qpx"], resident)
    assert ctx.get_option("errors") == 0


# ---- do_imaging at odd N ----------------------------------------------------------------------------------------------------------
def odd_case(lam, n, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.6, 0.6, n) * lam, rng.uniform(-0.6, 0.6, n) * lam  # some outside the grid, half with v < 0
    v[5::29] = 0.0
    v[::17] = -0.0
    return u, v, rng.uniform(-500, 500, n), rng.normal(size=n) + 1j * rng.normal(size=n)


def imaging_pair(kind, N, seed=10):
    """(the numpy oracle's imaging function, do_imaging's tuple for host arrays, the same for torch tensors)"""
    rng = np.random.default_rng(seed)
    kv = rng.normal(size=(2, 2, 7, 7)) + 1j * rng.normal(size=(2, 2, 7, 7))
    ko = dict(wstep=200, qpx=2, npixFF=32, npixKern=7)
    z = lambda: np.zeros((N, N), complex)  # noqa: E731
    if kind == "simple":
        return (lambda th, la, uu, vv, ww, vs: P.grid(z(), uu / la, vv / la, vs)), ("simple",), ("simple",)
    if kind == "conv":
        return (lambda th, la, uu, vv, ww, vs: P.convgrid(kv, z(), uu / la, vv / la, vs)), ("conv", kv), ("conv", to_dev(kv))
    return ((lambda th, la, uu, vv, ww, vs: P.w_cache_imaging(th, la, uu, vv, ww, vs, 200, 2, 32, 7)[0]),
            ("w_cache", ko), ("w_cache", ko))


def check_do_imaging(ctx, theta, lam, u, v, w, vis, fn, spec, dspec):
    import torch
    rimg, rpsf, rpmax = P.do_imaging(theta, lam, u, v, w, vis, fn)
    assert abs(rpsf.max() - 1.0) < 1e-12
    img, psf, pmax = ctx.do_imaging(theta, lam, (u, v, w), None, None, None, 1.0e8, vis, spec)
    dimg, dpsf, dpmax = ctx.do_imaging(theta, lam, to_dev(np.stack([u, v, w], 1)), None, None, None, 1.0e8, to_dev(vis),
                                       dspec)
    torch.cuda.synchronize()
    for i, p, m in ((img, psf, pmax), (dimg.cpu().numpy(), dpsf.cpu().numpy(), dpmax)):
        assert abs(m - rpmax) / abs(rpmax) < TOL
        assert rel(p, rpsf) < TOL and abs(p.max() - 1.0) < 1e-12
        assert rel(i, rimg) < TOL
    return rpsf


@pytest.mark.parametrize("kind", ["simple", "conv", "w_cache"])
@pytest.mark.parametrize("lam,N", [(2540, 127), (180, 9)])
def test_do_imaging_odd_n(ctx, kind, lam, N):
    """do_imaging with odd N, host form and resident form ((n, 3) torch matrix): the odd branch of hermitian_kernel with
    the roll s = N / 2 folded in, and real_max_kernel<false> reading at (N + 1) / 2 - the two rolls of the centred
    transform differ for odd N only.  Some baselines fall outside the grid (weight_cell returning -1 under do_imaging),
    half have v < 0 (mirrored) and some v == -0.0 or 0.0 (not mirrored)."""
    theta = 0.05
    assert ctx.image_size(theta, lam) == N == P.haskell_round(theta * lam) and N % 2 == 1
    u, v, w, vis = odd_case(lam, 800, 100 + N)
    assert (np.abs(u) > 0.52 * lam).sum() > 50 and np.signbit(v[::17]).all() and (v < 0).sum() > 300
    check_do_imaging(ctx, theta, lam, u, v, w, vis, *imaging_pair(kind, N))
    assert ctx.get_option("errors") == 0


def test_do_imaging_odd_n_psf_maximum_off_centre(ctx):
    """The ordered-bits maximum of real_max_kernel<false> against psf.max() of the oracle, not against an assumed
    position: five visibilities gridded with a random complex kernel give a "PSF" whose largest cell is not the centre
    cell (N = 127: the maximum is read through the folded roll (N + 1) / 2)."""
    theta, lam, N = 0.05, 2540, 127
    rng = np.random.default_rng(7)
    u, v = rng.uniform(-0.4, 0.4, 5) * lam, rng.uniform(-0.4, 0.4, 5) * lam
    w, vis = rng.uniform(-100, 100, 5), rng.normal(size=5) + 1j * rng.normal(size=5)
    rpsf = check_do_imaging(ctx, theta, lam, u, v, w, vis, *imaging_pair("conv", N, seed=11))
    assert np.unravel_index(np.argmax(rpsf), rpsf.shape) != (N // 2, N // 2)
