"""Every device implementation of the cell / sub-cell rule at exact ties and extremes (streams: tests/coord_cases.py,
whose structure tests/test_coord_cases_host.py establishes).

The tile gridders, `grid`, the weights' counts and uniform weights are compared bit for bit: kernel taps, visibilities
and degrid grids are small integers, so every sum is an integer far below 2^53 whatever the order of the atomics, and a
visibility binned to another cell or sub-cell changes the result by at least 1.  The aw gridders convolve their kernels
on the device and the imagers end in an FFT: those are compared at the project's 1e-10 (BASELINE.json's north star),
where a wrong cell or sub-cell is an O(1) error.

gridhip_last_dropped counts visibilities left out because of their w-plane, and only those with a tap inside the grid
(include/gridhip.h); one that has no tap inside the grid changes nothing and is not counted.  The streams therefore
carry w-planes W and -1 on tie coordinates whose cell is inside the grid: the count is theirs, and a visibility moved
off the grid by a wrong cell would be missing from it."""
import numpy as np
import pytest

import coord_cases as cc
import weights_ref
from oracle import gridref_np as P
from test_gpu_aw_degrid import awdegrid_np
from test_gpu_imager import KO, Case, against_the_calls, host, imgfn_of, kv_table, np_imgfn, rel, to_dev

pytestmark = pytest.mark.gpu

TOL, TIGHT = 1e-10, 1e-13
GRID_Q = [(H, Wd, Q) for H, Wd in cc.GRIDS for Q in cc.QS]
_refs = {}


def zeros(H, Wd):
    return np.zeros((H, Wd), dtype=np.complex128)


def refs(oracle, H, Wd, Q, gh, gw):
    """(stream, taps, degrid grid, the oracle's grid, the oracle's predictions): computed once, never changed"""
    key = (H, Wd, Q, gh, gw)
    if key not in _refs:
        if (H, Wd, Q) not in _refs:
            _refs[(H, Wd, Q)] = cc.tie_stream(H, Wd, Q)
        s = _refs[(H, Wd, Q)]
        g, G, k = cc.int_gcf(Q, gh, gw), cc.int_grid(H, Wd), s.keep
        grid = oracle.convgrid2(g, zeros(H, Wd), s.u[k], s.v[k], s.wb[k], s.vis[k])
        d = np.zeros(len(s.u), dtype=np.complex128)
        d[k] = oracle.degrid2(g, G, s.u[k], s.v[k], s.wb[k])
        for a in (grid, d):
            a.setflags(write=False)
        _refs[key] = (s, g, G, grid, d)
    return _refs[key]


def off8(a):
    """a device copy that starts 8 bytes off a 16-byte boundary: a view big[1:]"""
    import torch
    big = torch.zeros(len(a) + 1, dtype=torch.from_numpy(a[:1]).dtype, device="cuda:0")
    big[1:] = to_dev(a)
    assert big[1:].data_ptr() % 16 == 8
    return big[1:]


def coords(s, layout, sl=slice(None)):
    """(p, wbin) on the device in one of the three layouts"""
    u, v, wb = s.u[sl], s.v[sl], s.wb[sl]
    if layout == "aligned":
        p = (to_dev(u), to_dev(v), None)
        assert p[0].data_ptr() % 16 == 0 and p[1].data_ptr() % 16 == 0
        return p, to_dev(wb)
    if layout == "off8":
        return (off8(u), off8(v), None), off8(wb)
    return to_dev(np.stack([u, v, np.zeros(len(u))], axis=1)), to_dev(wb)


def options(ctx, **opts):
    class Scope:
        def __enter__(self):
            for k, val in opts.items():
                ctx.set_option(k, val)

        def __exit__(self, *exc):
            for k in opts:
                ctx.set_option(k, 0)
    return Scope()


def dev_pair(ctx, s, g, G, p, wb, sl=slice(None)):
    """convgrid2 and degrid2 in their device forms -> (grid, predictions, paths, dropped counts)"""
    import torch
    n = len(s.u[sl])
    tg = to_dev(g)
    out = torch.zeros(G.shape, dtype=torch.complex128, device="cuda:0")
    ctx.convgrid2(tg, out, p, wb, to_dev(s.vis[sl]))
    torch.cuda.synchronize()
    assert ctx.get_option("errors") == 0
    paths, drops = [ctx.get_option("last_path")], [ctx.last_dropped()]
    pred = torch.full((n,), float("nan"), dtype=torch.complex128, device="cuda:0")
    ctx.degrid2(tg, to_dev(G), p, wb, pred)
    torch.cuda.synchronize()
    assert ctx.get_option("errors") == 0
    return host(out), host(pred), paths + [ctx.get_option("last_path")], drops + [ctx.last_dropped()]


def path_of(gh, gw, sort, subfoot=0):
    """read-only option "last_path" for a forced "sort": 3 = general tile kernel, 1 = tap-reusing kernel, 2 = the same
    through sub-footprints (non-square supports, supports below 5, supports above 16 under "subfoot")"""
    if sort == 2:
        return 3
    return 1 if gh == gw and 5 <= gh <= 32 and not (subfoot and gh > 16) else 2


# ---- a. tile gridders, default options ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gh,gw", cc.SUPPORTS)
@pytest.mark.parametrize("H,Wd,Q", GRID_Q)
def test_tile_gridders_default_options(ctx, oracle, H, Wd, Q, gh, gw):
    import torch
    s, g, G, ref, dref = refs(oracle, H, Wd, Q, gh, gw)
    n = len(s.u)
    got = ctx.convgrid2(g, zeros(H, Wd), (s.u, s.v, None), s.wb, s.vis)
    assert ctx.get_option("errors") == 0 and ctx.last_dropped() == s.nbad
    assert np.array_equal(got, ref), (np.abs(got - ref).max(), int((got != ref).sum()))
    d = ctx.degrid2(g, G, (s.u, s.v, None), s.wb, out=np.full(n, np.nan + 1j * np.nan))
    assert ctx.get_option("errors") == 0 and ctx.last_dropped() == s.nbad
    assert np.array_equal(d, dref), int((d != dref).sum())
    plan = ctx.plan((H, Wd), g.shape, (to_dev(s.u), to_dev(s.v), None), to_dev(s.wb))
    pg = plan.grid(to_dev(g), torch.zeros((H, Wd), dtype=torch.complex128, device="cuda:0"), to_dev(s.vis))
    pd = plan.degrid(to_dev(g), to_dev(G), out=torch.full((n,), 7.0 + 7j, dtype=torch.complex128, device="cuda:0"))
    torch.cuda.synchronize()
    assert ctx.get_option("errors") == 0
    pg, pd = host(pg), host(pd)
    plan.close()
    assert np.array_equal(pg, ref), int((pg != ref).sum())
    assert np.array_equal(pd, dref), int((pd != dref).sum())


# ---- b. option matrix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["aligned", "off8", "matrix"])
@pytest.mark.parametrize("prepass", [0, 1, 2, 4, 5, 6])
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_prepass_and_coordinate_layout(ctx, oracle, H, Wd, Q, prepass, layout):
    s, g, G, ref, dref = refs(oracle, H, Wd, Q, 7, 7)
    p, wb = coords(s, layout)
    with options(ctx, prepass=prepass):
        got, d, _, drops = dev_pair(ctx, s, g, G, p, wb)
    assert drops == [s.nbad, s.nbad]
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert np.array_equal(d, dref), int((d != dref).sum())


@pytest.mark.parametrize("gh,gw", cc.SUPPORTS)
@pytest.mark.parametrize("sort", [0, 1, 2])
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_sort_option(ctx, oracle, H, Wd, Q, sort, gh, gw):
    s, g, G, ref, dref = refs(oracle, H, Wd, Q, gh, gw)
    p, wb = coords(s, "aligned")
    with options(ctx, sort=sort):
        got, d, paths, drops = dev_pair(ctx, s, g, G, p, wb)
    if sort:
        assert paths == [path_of(gh, gw, sort)] * 2
    assert drops == [s.nbad, s.nbad]
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert np.array_equal(d, dref), int((d != dref).sum())


@pytest.mark.parametrize("gh,gw", [(17, 17), (9, 5)])
@pytest.mark.parametrize("subfoot", [0, 1])
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_subfoot_option(ctx, oracle, H, Wd, Q, subfoot, gh, gw):
    s, g, G, ref, dref = refs(oracle, H, Wd, Q, gh, gw)
    p, wb = coords(s, "aligned")
    with options(ctx, sort=1, subfoot=subfoot, prepass=2):
        got, d, paths, drops = dev_pair(ctx, s, g, G, p, wb)
    assert paths == [path_of(gh, gw, 1, subfoot)] * 2
    assert drops == [s.nbad, s.nbad]
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert np.array_equal(d, dref), int((d != dref).sum())


@pytest.mark.parametrize("gh,gw", cc.SUPPORTS)
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_direct_variant(ctx, oracle, H, Wd, Q, gh, gw):
    s, g, _, ref, _ = refs(oracle, H, Wd, Q, gh, gw)
    with options(ctx, variant=1):
        got = ctx.convgrid2(g, zeros(H, Wd), (s.u, s.v, None), s.wb, s.vis)
        assert ctx.get_option("last_path") == 4 and ctx.last_dropped() == s.nbad
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("layout", ["aligned", "off8"])
@pytest.mark.parametrize("prepass", [1, 2])
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_odd_lengths_reach_the_pair_paths_tail(ctx, oracle, H, Wd, Q, prepass, layout):
    """an odd n, whose last visibility has no partner in the 16-byte reads, and n = 1; the last visibility of each is
    a tie (the streams hold nothing else)"""
    s, g, G, _, _ = refs(oracle, H, Wd, Q, 5, 5)
    n0 = len(s.u) - 1 - len(s.u) % 2      # odd
    for n in (n0, 1):
        sl = slice(0, n)
        k = s.keep[sl]
        ref = oracle.convgrid2(g, zeros(H, Wd), s.u[sl][k], s.v[sl][k], s.wb[sl][k], s.vis[sl][k])
        dref = np.zeros(n, dtype=np.complex128)
        dref[k] = oracle.degrid2(g, G, s.u[sl][k], s.v[sl][k], s.wb[sl][k])
        p, wb = coords(s, layout, sl)
        with options(ctx, prepass=prepass):
            got, d, _, _ = dev_pair(ctx, s, g, G, p, wb, sl)
        assert np.array_equal(got, ref) and np.array_equal(d, dref), n


# ---- c. bin reuse across a tie -------------------------------------------------------------------------------------------
@pytest.fixture
def rctx():
    """a context of its own, as in test_gpu_bin_reuse.py: the counters start at zero and nobody else's records are in it"""
    import gridhip
    c = gridhip.Context(0)
    c.set_option("prepass", 2)
    c.set_option("sort", 1)
    yield c
    c.close()


@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_bin_reuse_notices_a_one_ulp_step_across_a_tie(rctx, oracle, H, Wd, Q):
    """Grid p, overwrite the same device buffers with p' one double further, across a cell or sub-cell step, and grid
    again: the verify sweep must see that the records changed.  The same for degrid, going back."""
    import torch
    au, bu = cc.ulp_pairs(Wd, Q)
    av, bv = cc.ulp_pairs(H, Q)
    n = max(len(au), len(av))
    rng = np.random.default_rng(H + Q)
    perm = rng.permutation(n)
    ua, ub = np.resize(au, n)[perm], np.resize(bu, n)[perm]
    va, vb = np.resize(av, n), np.resize(bv, n)
    wb, vis = rng.integers(0, cc.W, n), cc.cint(rng, n)
    g, G = cc.int_gcf(Q, 7, 7), cc.int_grid(H, Wd)
    ref_a = oracle.convgrid2(g, zeros(H, Wd), ua, va, wb, vis)
    ref_b = oracle.convgrid2(g, zeros(H, Wd), ub, vb, wb, vis)
    assert not np.array_equal(ref_a, ref_b)
    du, dv, dwb, dvis, dg, dG = (to_dev(a) for a in (ua, va, wb, vis, g, G))

    def grid():
        out = torch.zeros((H, Wd), dtype=torch.complex128, device="cuda:0")
        rctx.convgrid2(dg, out, (du, dv, None), dwb, dvis)
        torch.cuda.synchronize()
        assert rctx.get_option("errors") == 0
        return host(out)

    def degrid():
        out = torch.full((n,), float("nan"), dtype=torch.complex128, device="cuda:0")
        rctx.degrid2(dg, dG, (du, dv, None), dwb, out)
        torch.cuda.synchronize()
        assert rctx.get_option("errors") == 0
        return host(out)

    assert np.array_equal(grid(), ref_a)
    du.copy_(to_dev(ub)), dv.copy_(to_dev(vb))
    assert np.array_equal(grid(), ref_b)
    rctx.synchronize()
    assert rctx.get_option("prepass_verified") >= 1 and rctx.get_option("prepass_reused") == 0
    assert np.array_equal(degrid(), oracle.degrid2(g, G, ub, vb, wb))
    du.copy_(to_dev(ua)), dv.copy_(to_dev(va))
    assert np.array_equal(degrid(), oracle.degrid2(g, G, ua, va, wb))
    assert np.array_equal(grid(), ref_a)


# ---- d. `grid` and the simple predictor ---------------------------------------------------------------------------------
def grid_stream(H, Wd):
    u, v = cc.grid_candidates(H, Wd), cc.grid_candidates(H, H)
    n = max(len(u), len(v))
    rng = np.random.default_rng(H + Wd)
    return rng.permutation(np.resize(u, n)), np.resize(v, n), cc.cint(rng, n)


@pytest.mark.parametrize("H,Wd", cc.GRIDS + ((33, 49),))
def test_grid_takes_n_from_the_height_for_both_axes(ctx, oracle, H, Wd):
    u, v, vis = grid_stream(H, Wd)
    ref = oracle.grid(zeros(H, Wd), u, v, vis)
    assert np.array_equal(ref, P.grid(zeros(H, Wd), u, v, vis)) and ref.any()
    got = ctx.grid(zeros(H, Wd), (u, v, None), vis)
    assert np.array_equal(got, ref), int((got != ref).sum())
    import torch
    out = torch.zeros((H, Wd), dtype=torch.complex128, device="cuda:0")
    ctx.grid(out, to_dev(np.stack([u, v, np.zeros(len(u))], axis=1)), to_dev(vis))
    assert np.array_equal(host(out), ref)


def simple_gather(N, lam, model, u, v):
    """the simple kind's prediction: fft_c(model) at the cell floor(0.5 + N p), exactly 0 off the grid and for NaN"""
    F = P.fft_c(model.astype(np.complex128))
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = cc.grid_rule(N, u / np.float64(lam)), cc.grid_rule(N, v / np.float64(lam))
        ok = (fx >= -(N // 2)) & (fx < N - N // 2) & (fy >= -(N // 2)) & (fy < N - N // 2)
    out = np.zeros(len(u), dtype=np.complex128)
    out[ok] = F[N // 2 + fy[ok].astype(np.int64), N // 2 + fx[ok].astype(np.int64)]
    return out


@pytest.mark.parametrize("N", [49, 64])
def test_simple_predictors(ctx, N):
    theta, lam = 0.25, 4 * N
    assert ctx.image_size(theta, lam) == N
    u0 = cc.wavelengths(cc.grid_candidates(N, N), lam)
    rng = np.random.default_rng(N)
    u, v = rng.permutation(u0), u0.copy()
    w = np.zeros(len(u))
    model = rng.normal(size=(N, N))
    want = simple_gather(N, lam, model, u, v)
    assert (want == 0).sum() >= 10 and (want != 0).sum() >= 100
    got = ctx.predict(theta, lam, (u, v, w), model, ("simple",))
    assert ctx.get_option("errors") == 0
    assert np.array_equal(got == 0, want == 0) and rel(got, want) < TOL
    duvw = tuple(to_dev(a) for a in (u, v, w))
    im = ctx.imager(theta, lam, duvw, ("simple",))
    got = host(im.predict(to_dev(model)))
    im.close()
    assert np.array_equal(got == 0, want == 0) and rel(got, want) < TOL


# ---- e. aw -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [0, 2])
@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_aw_gridders_on_tie_streams(ctx, oracle, H, Wd, Q, cache, sort):
    S, A = 7, 3
    s = refs(oracle, H, Wd, Q, 7, 7)[0]
    step = max(1, len(s.u) // 700)
    u, v = s.u[::step], s.v[::step]
    n = len(u)
    key = ("aw", H, Wd, Q)
    if key not in _refs:
        rng = np.random.default_rng(H * Q)
        wk = rng.normal(size=(cc.W, Q, Q, S, S)) + 1j * rng.normal(size=(cc.W, Q, Q, S, S))
        ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
        wb, a1, a2 = rng.integers(0, cc.W, n), rng.integers(0, A, n), rng.integers(0, A, n)
        vis = rng.normal(size=n) + 1j * rng.normal(size=n)
        G = rng.normal(size=(H, Wd)) + 1j * rng.normal(size=(H, Wd))
        ref = oracle.awgrid(wk, ak, zeros(H, Wd), u, v, wb, a1, a2, vis, direct=True)
        dref = awdegrid_np(wk, ak, G, u, v, wb, a1, a2)
        _, xf, _, yf = P.frac_coords((H, Wd), Q, u, v)
        nkeys = len(set(zip(a1.tolist(), a2.tolist(), wb.tolist(), yf.tolist(), xf.tolist())))
        _refs[key] = (wk, ak, wb, a1, a2, vis, G, ref, dref, nkeys)
    wk, ak, wb, a1, a2, vis, G, ref, dref, nkeys = _refs[key]
    with options(ctx, sort=sort):
        try:
            ctx.set_option("aw_cache", cache)
            got = ctx.convgrid4(wk, ak, zeros(H, Wd), (u, v, None), (wb, a1, a2), vis)
            assert ctx.get_option("errors") == 0 and ctx.last_dropped() == 0
            assert ctx.get_option("last_path") == (3 if sort == 2 else 1)
            built = ctx.aw_stats(S)["kernels_built"]
            d = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2), out=np.full(n, np.nan + 1j * np.nan))
            assert ctx.get_option("errors") == 0 and ctx.get_option("last_path") == (3 if sort == 2 else 1)
        finally:
            ctx.set_option("aw_cache", 1)
    print(f"aw {H}x{Wd} Q={Q} cache={cache} sort={sort}: grid {rel(got, ref):.2e} degrid {rel(d, dref):.2e}, {built} kernels")
    assert rel(got, ref) < TOL and rel(d, dref) < TOL
    assert built == (nkeys if cache else n)


# ---- f. weights -----------------------------------------------------------------------------------------------------------
def weight_stream(N, extra=()):
    lam = 4 * N
    u0 = np.concatenate([cc.wavelengths(cc.candidates(N, 1), lam), np.asarray(extra, dtype=np.float64)])
    rng = np.random.default_rng(3 * N)
    return lam, rng.permutation(u0), u0.copy()


def weight_forms(u, v):
    """name -> p: host, device aligned, device 8 bytes off, device (n, 3) matrix"""
    return {"host": (u, v, None), "aligned": (to_dev(u), to_dev(v)), "off8": (off8(u), off8(v)),
            "stride3": to_dev(np.stack([u, v, np.zeros(len(u))], axis=1))}


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("N", [33, 49, 64, 100])
def test_weights_on_tie_streams(ctx, N, odd):
    theta = 0.25
    lam, u, v = weight_stream(N)
    n = len(u) - (len(u) % 2 == (0 if odd else 1))
    u, v = u[:n], v[:n]
    assert n % 2 == odd and ctx.image_size(theta, lam) == N
    for name, p in weight_forms(u, v).items():
        for mode in ("uniform", "natural", "briggs"):
            rw, rst, _ = weights_ref.weights(N, lam, u, v, mode, 0.5)
            w, st = ctx.weights(theta, lam, p, mode, 0.5)
            w, st = (host(w), host(st)) if name != "host" else (w, st)
            assert ctx.get_option("errors") == 0
            assert np.array_equal(st[5:], rst[5:]), (name, mode, st, rst)
            assert rst[5] >= 100 and rst[7] >= 10
            if mode == "uniform":
                assert np.array_equal(w, rw), (name, int((w != rw).sum()))
            else:
                assert np.all(np.abs(w - rw) <= TIGHT * np.abs(rw)), (name, mode)
            k = [0, 1, 2, 4]     # sum w, sum w^2 / s, sum s, f^2
            assert np.all(np.abs(st[k] - rst[k]) <= TIGHT * np.abs(rst[k])), (name, mode, st, rst)
    vis = cc.cint(np.random.default_rng(N), n)
    got = ctx.doweight(theta, lam, (u, v), vis)
    want = P.doweight(N, u / np.float64(lam), v / np.float64(lam), vis)
    assert np.array_equal(got, want), int((got != want).sum())


# ---- g. imagers ---------------------------------------------------------------------------------------------------------
def imager_case(ctx, kind, theta, lam):
    N = P.haskell_round(theta * lam)
    Q = {"simple": 1, "conv": 4, "w_cache": KO["qpx"]}[kind]
    base = cc.grid_candidates(N, N) if kind == "simple" else cc.candidates(N, Q)
    u0 = np.concatenate([cc.wavelengths(base, lam), [0.0, -0.0]])
    rng = np.random.default_rng(N + Q)
    u, v = rng.permutation(u0), u0.copy()
    n = len(u)
    assert (v == 0).sum() >= 2 and np.signbit(v[v == 0]).any() and (v > 0).sum() > 100 and (v < 0).sum() > 100
    c = Case.__new__(Case)
    c.ctx, c.kind, c.theta, c.lam, c.N = ctx, kind, theta, lam, N
    c.uvw = (u, v, rng.uniform(-100.0, 100.0, n))
    c.vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    c.model = rng.normal(size=(N, N))
    c.kv, c.aw = (kv_table(4, 7, N) if kind == "conv" else None), None
    c.bind()
    return c


@pytest.mark.parametrize("theta,lam", [(0.1, 490), (0.1, 640)])     # N = 49 and N = 64
@pytest.mark.parametrize("kind", ["simple", "conv", "w_cache"])
def test_imagers_on_tie_streams(ctx, kind, theta, lam):
    c = imager_case(ctx, kind, theta, lam)
    assert ctx.image_size(theta, lam) == c.N
    against_the_calls(c)
    if kind != "w_cache":   # a uniform-weighted imager's psf against numpy's do_imaging
        u, v, w = c.uvw
        _, psf_ref, pmax_ref = P.do_imaging(theta, lam, u, v, w, c.vis, np_imgfn(kind, kv=c.kv))
        assert pmax_ref > 0 and rel(host(c.im.psf), psf_ref) < TOL
    assert ctx.get_option("errors") == 0
    c.im.close()


# ---- h. extremes ------------------------------------------------------------------------------------------------------------
def extreme_pairs(nu, nv, S):
    """every extreme on one axis with a coordinate at the grid's centre on the other, then extremes on both; the
    oracle-side rule: a visibility counts for something only when both cells are finite and their footprints touch"""
    eu, ev = cc.extremes(nu, S), cc.extremes(nv, S)
    u = np.concatenate([eu, np.zeros(len(ev)), eu])
    v = np.concatenate([np.zeros(len(eu)), ev, np.resize(ev[::-1], len(eu))])
    return u, v


def touching(H, Wd, Q, gh, gw, u, v):
    with np.errstate(invalid="ignore", over="ignore"):
        cx = np.floor((np.float64(Wd // 2) + u * np.float64(Wd)) + 0.5 / Q)
        cy = np.floor((np.float64(H // 2) + v * np.float64(H)) + 0.5 / Q)
    return cc.touches(Wd, gw, cx) & cc.touches(H, gh, cy)


@pytest.mark.parametrize("gh,gw", cc.SUPPORTS)
@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_extremes_through_the_gridders(ctx, oracle, H, Wd, Q, gh, gw):
    import torch
    u, v = extreme_pairs(Wd, H, max(gh, gw))
    n = len(u)
    t = touching(H, Wd, Q, gh, gw, u, v)
    assert t.sum() >= 10 and (~t).sum() >= 30
    rng = np.random.default_rng(n)
    wb, vis = rng.integers(0, cc.W, n), cc.cint(rng, n)
    far = ~(np.abs(u) <= 1) | ~(np.abs(v) <= 1)
    assert not (far & t).any() and far.sum() >= 20
    wb[np.flatnonzero(far)[::3]] = cc.W     # far off the grid (or NaN) and a bad w-plane: not counted
    g, G = cc.int_gcf(Q, gh, gw), cc.int_grid(H, Wd)
    ref = oracle.convgrid2(g, zeros(H, Wd), u[t], v[t], wb[t], vis[t])
    dref = np.zeros(n, dtype=np.complex128)
    dref[t] = oracle.degrid2(g, G, u[t], v[t], wb[t])
    for opts in ({}, {"prepass": 2, "sort": 1}, {"sort": 2}, {"variant": 1}):
        with options(ctx, **opts):
            got = ctx.convgrid2(g, zeros(H, Wd), (u, v, None), wb, vis)
            assert ctx.get_option("errors") == 0 and ctx.last_dropped() == 0
            assert np.array_equal(got, ref), opts
            if "variant" not in opts:
                d = ctx.degrid2(g, G, (u, v, None), wb, out=np.full(n, np.nan + 1j * np.nan))
                assert ctx.get_option("errors") == 0 and ctx.last_dropped() == 0
                assert np.array_equal(d, dref) and not d[~t].any(), opts
    plan = ctx.plan((H, Wd), g.shape, (to_dev(u), to_dev(v), None), to_dev(wb))
    pg = plan.grid(to_dev(g), torch.zeros((H, Wd), dtype=torch.complex128, device="cuda:0"), to_dev(vis))
    pd = plan.degrid(to_dev(g), to_dev(G), out=torch.full((n,), float("nan"), dtype=torch.complex128, device="cuda:0"))
    torch.cuda.synchronize()
    assert np.array_equal(host(pg), ref) and np.array_equal(host(pd), dref)
    plan.close()


@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_extremes_through_the_aw_gridders(ctx, oracle, H, Wd, Q):
    S, A = 7, 2
    u, v = extreme_pairs(Wd, H, S)
    n = len(u)
    t = touching(H, Wd, Q, S, S, u, v)
    rng = np.random.default_rng(n + Q)
    wk = rng.normal(size=(cc.W, Q, Q, S, S)) + 1j * rng.normal(size=(cc.W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    wb, a1, a2 = rng.integers(0, cc.W, n), rng.integers(0, A, n), rng.integers(0, A, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    G = rng.normal(size=(H, Wd)) + 1j * rng.normal(size=(H, Wd))
    ref = oracle.awgrid(wk, ak, zeros(H, Wd), u[t], v[t], wb[t], a1[t], a2[t], vis[t], direct=True)
    dref = np.zeros(n, dtype=np.complex128)
    dref[t] = awdegrid_np(wk, ak, G, u[t], v[t], wb[t], a1[t], a2[t])
    try:
        for cache in (1, 0):
            ctx.set_option("aw_cache", cache)
            got = ctx.convgrid4(wk, ak, zeros(H, Wd), (u, v, None), (wb, a1, a2), vis)
            assert ctx.get_option("errors") == 0
            d = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2), out=np.full(n, np.nan + 1j * np.nan))
            assert ctx.get_option("errors") == 0
            assert np.isfinite(got).all() and rel(got, ref) < TOL
            assert np.isfinite(d).all() and not d[~t].any() and rel(d, dref) < TOL
    finally:
        ctx.set_option("aw_cache", 1)


@pytest.mark.parametrize("H,Wd", [(49, 33), (100, 257)])
def test_extremes_through_grid(ctx, oracle, H, Wd):
    u, v = extreme_pairs(Wd, H, 1)
    # (`grid` bins both axes with H)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = cc.grid_rule(H, u), cc.grid_rule(H, v)
        t = (fx >= -(H // 2)) & (fx < Wd - H // 2) & (fy >= -(H // 2)) & (fy < H - H // 2)
    vis = cc.cint(np.random.default_rng(H), len(u))
    ref = oracle.grid(zeros(H, Wd), u[t], v[t], vis[t])
    got = ctx.grid(zeros(H, Wd), (u, v, None), vis)
    assert t.sum() >= 4 and np.array_equal(got, ref)


@pytest.mark.parametrize("N", [49, 64])
def test_extremes_through_weights_and_predictors(ctx, N):
    theta, lam = 0.25, 4 * N
    e = cc.extremes(N, 1) * lam
    u, v = np.concatenate([e, np.zeros(len(e)), e]), np.concatenate([np.zeros(len(e)), e, e[::-1]])
    n = len(u)
    for name, p in weight_forms(u, v).items():
        for mode in ("uniform", "natural", "briggs"):
            rw, rst, _ = weights_ref.weights(N, lam, u, v, mode, 0.5)
            w, st = ctx.weights(theta, lam, p, mode, 0.5)
            w, st = (host(w), host(st)) if name != "host" else (w, st)
            assert np.array_equal(st[5:], rst[5:]) and rst[7] >= 30 and rst[5] >= 4, (name, mode, st, rst)
            assert np.isfinite(w).all() and np.all(np.abs(w - rw) <= TIGHT * np.abs(rw)), (name, mode)
            outside = weights_ref.cells(N, lam, u, v) < 0
            assert np.all(w[outside] == 1.0)          # unchanged s t
    vis = cc.cint(np.random.default_rng(N), n)
    got = ctx.doweight(theta, lam, (u, v), vis)
    with np.errstate(invalid="ignore", over="ignore"):
        c = weights_ref.cells(N, lam, u, v)
    want = vis.copy()
    inside = c >= 0
    want[inside] = vis[inside] / np.bincount(c[inside], minlength=N * N)[c[inside]]
    assert np.array_equal(got, want)
    model = np.random.default_rng(N + 1).normal(size=(N, N))
    pred_ref = simple_gather(N, lam, model, u, v)
    pred = ctx.predict(theta, lam, (u, v, np.zeros(n)), model, ("simple",))
    assert np.isfinite(pred).all() and np.array_equal(pred == 0, pred_ref == 0) and rel(pred, pred_ref) < TOL
    for kind, kv in (("conv", kv_table(4, 7, N)), ("w_cache", None)):
        Q, S = (4, 7) if kind == "conv" else (KO["qpx"], KO["npixKern"])
        pred = ctx.predict(theta, lam, (u, v, np.zeros(n)), model, imgfn_of(kind, kv))
        t = touching(N, N, Q, S, S, u / np.float64(lam), v / np.float64(lam))
        assert ctx.get_option("errors") == 0 and np.isfinite(pred).all() and not pred[~t].any() and pred[t].any(), kind
    duvw = tuple(to_dev(a) for a in (u, v, np.zeros(n)))
    for kind, kv in (("simple", None), ("conv", to_dev(kv_table(4, 7, N)))):
        im = ctx.imager(theta, lam, duvw, imgfn_of(kind, kv))
        pred = host(im.predict(to_dev(model)))
        img = host(im.cycle(to_dev(vis)))
        assert np.isfinite(pred).all() and np.isfinite(img).all() and np.isfinite(host(im.psf)).all(), kind
        if kind == "simple":
            assert np.array_equal(pred == 0, pred_ref == 0) and rel(pred, pred_ref) < TOL
        im.close()
