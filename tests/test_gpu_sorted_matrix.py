"""Every instantiation and run shape of tile_grid_sorted_kernel (csrc/tile_sorted.hip) against the oracle.

The kernel is compiled 136 ways.  Each one is run here with the kernel forced on ("sort" = 1), and every call is
followed by `errors == 0` and `last_path == 1` (and `last_bigtile` where it applies), so no test passes on a fall-back
to the general tile kernel.

    instantiation                                   run by
    <S, grid,   classic tile>  S = 5..32            test_classic_tile_small_grid[S-*], test_production_tile[S-*-*]
    <S, degrid, classic tile>  S = 5..32            the same tests (degrid2 and a plan's degrid in each)
    <S, grid,   BT>            S = 5..32            test_big_tile[S]
    <S, degrid, BT>            S = 5..32            test_big_tile[S]
    <S, grid,   aw>            S = 5..16            test_aw_form[S]  (convgrid4)
    <S, degrid, aw>            S = 5..16            test_aw_form[S]  (degrid4)

Part B (seeded streams, 1e-10 of max|ref|, BASELINE.json's north star): the classic tile with the tiny tile a small
grid gets and with the tile and 15 walkers of a large grid under each table of walker weights, the big tile, the aw form.
Part C (test_structured_*): streams of sorted_cases.py built to reach the walker's control flow on purpose, with
small-integer values, so that the comparison is np.array_equal whatever the order of the atomics
(test_sorted_cases_host.py proves the exactness and each stream's structure on the CPU).  The aw streams keep the
tolerance: an aw kernel is a convolution of three tables, evaluated through FFTs by the reference."""
import contextlib
import functools

import numpy as np
import pytest

import sorted_cases as K
from oracle import gridref_np as P

pytestmark = pytest.mark.gpu
TOL = 1e-10
NAN = complex("nan+nanj")
SENTINEL = 7.0 + 1.0j


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def full(n, value):
    import torch
    return torch.full((n,), value, dtype=torch.complex128, device="cuda:0")


def zeros(H, Wd):
    import torch
    return torch.zeros((H, Wd), dtype=torch.complex128, device="cuda:0")


@contextlib.contextmanager
def options(ctx, **opts):
    try:
        for k, val in opts.items():
            ctx.set_option(k, val)
        yield
    finally:
        for k in opts:
            ctx.set_option(k, 0)


def prod_geometry(S, block=1024, **more):
    tx, ty = K.PROD_TILE[S]
    return dict(sort=1, tile_x=tx, tile_y=ty, block=block, **more)


def sorted_ran(ctx, tile=None, bigtile=None):
    """what every call of this module is followed by: the tap-reusing kernel ran, one record per visibility, and its
    sorter and walkers met nothing inconsistent"""
    assert ctx.get_option("errors") == 0
    assert ctx.get_option("last_path") == 1
    if tile is not None:
        assert (ctx.get_option("last_tile_x"), ctx.get_option("last_tile_y")) == tuple(tile)
    if bigtile is not None:
        assert ctx.get_option("last_bigtile") == bigtile


def four_calls(ctx, H, Wd, gcf, G, u, v, wb, vis, grid=None, **expect):
    """convgrid2, degrid2 into an output of NaNs, and a plan's grid and degrid (into an output of another sentinel: where
    a visibility's parts are summed with atomics the result must not depend on what the output held).  `G`, `grid`: the
    degrid input and a zeroed grid already on the device, or None."""
    n = len(u)
    tg, tu, tv, twb, tvis = t(gcf), t(u), t(v), t(wb), t(vis)
    tG = t(G) if isinstance(G, np.ndarray) else G
    g1 = ctx.convgrid2(tg, zeros(H, Wd) if grid is None else grid, (tu, tv, None), twb, tvis)
    sorted_ran(ctx, **expect)
    dropped = ctx.last_dropped()
    d1 = ctx.degrid2(tg, tG, (tu, tv, None), twb, full(n, NAN))
    sorted_ran(ctx, **expect)
    plan = ctx.plan((H, Wd), gcf.shape, (tu, tv, None), twb)
    g2 = None
    if grid is None:
        g2 = plan.grid(tg, zeros(H, Wd), tvis)
        sorted_ran(ctx, **expect)
    d2 = plan.degrid(tg, tG, full(n, SENTINEL))
    sorted_ran(ctx, **expect)
    plan.close()
    return g1, d1, g2, d2, dropped


# ---- B1 / B2: the classic tile -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_case(S, density, oracle):
    """the stream of B1 and B2 and its references, computed once"""
    W, Q = K.DENSITIES[density]
    gcf, u, v, wb, vis = K.uniform_case(S, K.H1, K.WD1, W, Q, S, K.N1, K.SPREAD1)
    G = np.random.default_rng(S + 100).normal(size=(2, K.H1, K.WD1))
    G = G[0] + 1j * G[1]
    ref = oracle.convgrid2(gcf, np.zeros((K.H1, K.WD1), dtype=np.complex128), u, v, wb, vis, mt_mode=2)
    dref = oracle.degrid2(gcf, G, u, v, wb)
    for a in (gcf, u, v, wb, vis, G, ref, dref):
        a.setflags(write=False)
    return gcf, u, v, wb, vis, G, ref, dref


def check_matrix(ctx, oracle, S, density, **expect):
    gcf, u, v, wb, vis, G, ref, dref = matrix_case(S, density, oracle)
    g1, d1, g2, d2, _ = four_calls(ctx, K.H1, K.WD1, gcf, G, u, v, wb, vis, **expect)
    errs = [rel(g1.cpu().numpy(), ref), rel(g2.cpu().numpy(), ref), rel(d1.cpu().numpy(), dref), rel(d2.cpu().numpy(), dref)]
    print(S, density, expect, errs)
    assert (dref == 0).any()      # footprints wholly outside the grid: their predictions are written as zeros
    for d in (d1, d2):
        assert np.isfinite(d.cpu().numpy()).all() and not d.cpu().numpy()[dref == 0].any()
    assert max(errs) < TOL


@pytest.mark.parametrize("density", list(K.DENSITIES))
@pytest.mark.parametrize("S", K.SUPPORTS)
def test_classic_tile_small_grid(ctx, oracle, S, density):
    """B1: the geometry a small grid gets by default - 16 x 16 tiles - with long and with short runs"""
    with options(ctx, sort=1):
        check_matrix(ctx, oracle, S, density, tile=(K.SMALL_TILE,) * 2, bigtile=0)


@pytest.fixture(scope="module")
def big(ctx):
    """B3's grid, on the device once: a zeroed 3200 x 3200 grid (every test leaves it zeroed) and a degrid input"""
    import torch
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(3200)
    G = torch.complex(*(torch.randn(K.N3, K.N3, generator=gen, device="cuda:0", dtype=torch.float64) for _ in range(2)))
    return {"grid": zeros(K.N3, K.N3), "G": G, "Ghost": G.cpu().numpy(), "host": np.zeros((K.N3, K.N3), dtype=np.complex128)}


def test_production_tile_table_matches_the_library(ctx, big):
    """The tile a grid with room for 1024 of them gets, one probe call per support (one visibility, default options):
    equal to the literal table B2 and C use, so that a change of the geometry rule is noticed."""
    got = {}
    for S in K.SUPPORTS:
        gcf = np.ones((K.W3, K.Q3, K.Q3, S, S), dtype=np.complex128)
        ctx.convgrid2(t(gcf), big["grid"], (t(np.zeros(1)), t(np.zeros(1)), None), t(np.zeros(1, dtype=np.int64)),
                      t(np.ones(1, dtype=np.complex128)))
        got[S] = (ctx.get_option("last_tile_x"), ctx.get_option("last_tile_y"))
        assert ctx.get_option("last_bigtile") == 0
    big["grid"].zero_()
    assert got == K.PROD_TILE


@pytest.mark.parametrize("density", list(K.DENSITIES))
@pytest.mark.parametrize("wtable", [1, 2, 3])
@pytest.mark.parametrize("S", K.SUPPORTS)
def test_production_tile(ctx, oracle, S, wtable, density):
    """B2: the tile and the 15 walkers of a large grid on the small one - a few tiles of thousands of records each -
    under each table of walker weights (cut15[0..2]: flat, steep, big-tile)"""
    with options(ctx, **prod_geometry(S, wtable=wtable)):
        check_matrix(ctx, oracle, S, density, tile=K.PROD_TILE[S], bigtile=0)


# ---- B3: the big tile -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", K.SUPPORTS)
def test_big_tile(ctx, oracle, big, S):
    """B3: option "bigtile" = 1 on a grid with room for 1024 big tiles; visibilities in a window at the grid's corner (the
    flush clips, the tile load fills with zeros) and one at the centre.  Whether the support gets the big tile is
    recorded in K.BIGTILE_SUPPORTS; the others must still take the tap-reusing kernel."""
    import torch
    gcf, u, v, wb, vis, side = K.window_case(S, S)
    lo, hi, c = 0, side + S + 1, K.N3 // 2
    clo, chi = c - side // 2 - S - 1, c + side // 2 + S + 1
    wins = [(slice(lo, hi), slice(lo, hi)), (slice(clo, chi), slice(clo, chi))]
    ref = oracle.convgrid2(gcf, big["host"], u, v, wb, vis, mt_mode=2)
    try:
        assert np.count_nonzero(ref) == sum(np.count_nonzero(ref[w]) for w in wins)
        dref = oracle.degrid2(gcf, big["Ghost"], u, v, wb)
        bt = int(S in K.BIGTILE_SUPPORTS)
        with options(ctx, sort=1, bigtile=1):
            g1, d1, _, d2, _ = four_calls(ctx, K.N3, K.N3, gcf, big["G"], u, v, wb, vis, grid=big["grid"], bigtile=bt)
        nz = lambda a: int(torch.count_nonzero(torch.view_as_real(a)))   # noqa: E731
        assert nz(g1) == sum(nz(g1[w]) for w in wins)                     # nothing outside the two windows
        scale = np.abs(ref).max()
        errs = [np.abs(g1[w].cpu().numpy() - ref[w]).max() / scale for w in wins]
        errs += [rel(d1.cpu().numpy(), dref), rel(d2.cpu().numpy(), dref)]
        print(S, bt, errs)
        assert max(errs) < TOL
    finally:
        big["grid"].zero_()
        for w in wins:
            big["host"][w] = 0


def test_big_tile_supports_are_the_recorded_set(ctx, big):
    """which supports really get the big tile at this grid: equal to the recorded literal, which holds the four that
    test_gpu_parity.py establishes"""
    got = set()
    with options(ctx, sort=1, bigtile=1):
        for S in K.SUPPORTS:
            gcf = np.ones((K.W3, K.Q3, K.Q3, S, S), dtype=np.complex128)
            ctx.convgrid2(t(gcf), big["grid"], (t(np.zeros(1)), t(np.zeros(1)), None), t(np.zeros(1, dtype=np.int64)),
                          t(np.ones(1, dtype=np.complex128)))
            sorted_ran(ctx)
            if ctx.get_option("last_bigtile"):
                got.add(S)
    big["grid"].zero_()
    assert {9, 15, 17, 21} <= K.BIGTILE_SUPPORTS and got == K.BIGTILE_SUPPORTS


# ---- B4 and the aw streams ---------------------------------------------------------------------------------------------
def aw_refs(wk, ak, H, Wd, u, v, wb, a1, a2, vis, G):
    """convgrid4 and its gather restated with numpy (oracle/gridref_np.aw_kernel_fn2; the gather as
    test_gpu_aw_degrid.awdegrid_np has it), one kernel per distinct (a1, a2, wbin, yf, xf), built once for both"""
    W, Q, _, S, _ = wk.shape
    A = ak.shape[0]
    ok = np.isfinite(u) & np.isfinite(v) & (wb >= 0) & (wb < W) & (a1 >= 0) & (a1 < A) & (a2 >= 0) & (a2 < A)
    x, xf, y, yf = P.frac_coords((H, Wd), Q, np.where(ok, u, 0.0), np.where(ok, v, 0.0))
    grid, out, kern = np.zeros((H, Wd), dtype=np.complex128), np.zeros(len(u), dtype=np.complex128), {}
    for k in np.flatnonzero(ok):
        key = (int(wb[k]), int(yf[k]), int(xf[k]), int(a1[k]), int(a2[k]))
        if key not in kern:
            kern[key] = np.conj(P.aw_kernel_fn2(key[1], key[2], wk[key[0]], ak[key[3]], ak[key[4]]))
        ys, xs = np.arange(S) + (y[k] - S // 2), np.arange(S) + (x[k] - S // 2)
        my, mx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < Wd)
        kk = kern[key][np.ix_(my, mx)]
        grid[np.ix_(ys[my], xs[mx])] += vis[k] * kk
        out[k] = (kk * G[np.ix_(ys[my], xs[mx])]).sum()
    return grid, out, len(kern)


def aw_calls(ctx, H, Wd, wk, ak, u, v, wb, a1, a2, vis, G):
    g = ctx.convgrid4(wk, ak, np.zeros((H, Wd), dtype=np.complex128), (u, v, None), (wb, a1, a2), vis)
    sorted_ran(ctx)
    d = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2), out=np.full(len(u), NAN))
    sorted_ran(ctx)
    return g, d


@pytest.mark.parametrize("S", K.AW_SUPPORTS)
def test_aw_form(ctx, S):
    """B4: convgrid4 and degrid4 at every support of the aw form, on a grid small enough for the oracle and with enough
    visibilities that the tile kernel is the tap-reusing one - which `last_path` now says after gridding too"""
    wk, ak, u, v, wb, a1, a2, vis, G = K.aw_case(S, K.H4, K.WD4, K.W4, K.Q4, S, K.A4, K.N4)
    ref, dref, _ = aw_refs(wk, ak, K.H4, K.WD4, u, v, wb, a1, a2, vis, G)
    g, d = aw_calls(ctx, K.H4, K.WD4, wk, ak, u, v, wb, a1, a2, vis, G)
    print(S, rel(g, ref), rel(d, dref))
    assert rel(g, ref) < TOL and np.isfinite(d).all() and rel(d, dref) < TOL


def test_aw_residues_share_histogram_slots(ctx):
    """C 8: more than 8192 distinct kernels in one batch and one tile: kernels k and k + 4096 share a slot of the sort's
    histogram and interleave in the sorted list, so runs end where the kernel index changes, not the slot.  Tolerance
    1e-10: aw kernels are convolutions of three tables, integers would not stay exact at 15 x 15."""
    wk, ak, u, v, wb, a1, a2, vis, G = K.aw_residues()
    ref, dref, D = aw_refs(wk, ak, K.H4, K.WD4, u, v, wb, a1, a2, vis, G)
    assert D >= 2 * K.AW_KEYS
    g, d = aw_calls(ctx, K.H4, K.WD4, wk, ak, u, v, wb, a1, a2, vis, G)
    assert ctx.get_option("aw_tables_built") == 1          # one batch
    print(D, rel(g, ref), rel(d, dref))
    assert rel(g, ref) < TOL and np.isfinite(d).all() and rel(d, dref) < TOL


# ---- C: structured streams, exact ------------------------------------------------------------------------------------
GEOMETRIES = ("default", "block64", "block128", "block1024")
STREAMS = {s.name: s for s in K.structured_streams()}


def geometry(name, S):
    return dict(sort=1) if name == "default" else prod_geometry(S, block=int(name[5:]))


@functools.lru_cache(maxsize=None)
def stream_refs(S, name, oracle):
    """a structured stream with its integer tables and the oracle's (exact) results; dropped records predict 0"""
    if name.startswith("window"):
        tx, ty = name[7:].split("x")
        s = K.window((int(tx), int(ty)), S)
    else:
        s = STREAMS[name]
    n = len(s.u)
    gcf, vis, G = K.int_tables(S, s.W, s.Q, n)
    keep = np.isfinite(s.u) & np.isfinite(s.v) & (s.wb < s.W)
    ref = oracle.convgrid2(gcf, np.zeros((K.HC, K.WDC), dtype=np.complex128), s.u[keep], s.v[keep], s.wb[keep], vis[keep])
    dref = np.zeros(n, dtype=np.complex128)
    dref[keep] = oracle.degrid2(gcf, G, s.u[keep], s.v[keep], s.wb[keep])
    return s, gcf, vis, G, ref, dref, keep


def check_exact(ctx, oracle, S, name, opts, **expect):
    s, gcf, vis, G, ref, dref, keep = stream_refs(S, name, oracle)
    with options(ctx, **{**opts, **s.opts}):
        g1, d1, g2, d2, dropped = four_calls(ctx, K.HC, K.WDC, gcf, G, s.u, s.v, s.wb, vis, **expect)
        if "wgroups" in s.opts:
            assert ctx.get_option("last_wgroups") == min(s.opts["wgroups"], s.W)
    assert dropped == (1 if s.ndrop else 0), name            # (wbin = W is counted; NaN coordinates are off the grid)
    bad = [what for what, got, want in (("convgrid2", g1, ref), ("plan.grid", g2, ref), ("degrid2", d1, dref),
                                        ("plan.degrid", d2, dref)) if not np.array_equal(got.cpu().numpy(), want)]
    assert not bad, (name, bad)
    assert not d1.cpu().numpy()[~keep].any() and not d2.cpu().numpy()[~keep].any()


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("S", K.CLASS_SUPPORTS)
def test_structured_streams_exact(ctx, oracle, S, geom):
    """C 1 - 5, 7: one run of 1 .. 1000 records, runs of length 1 only, ladders of run lengths, items smaller than the
    walkers, items and batches under "chunk" = 64, w-groups that do not divide W - bit for bit, in both directions, under
    the default geometry and under the production tile with one wave, one walker and 15 walkers"""
    opts = geometry(geom, S)
    tile = None if geom == "default" else K.PROD_TILE[S]
    failed = []
    for s in STREAMS.values():
        try:
            check_exact(ctx, oracle, S, s.name, opts, tile=tile)
        except AssertionError as e:
            failed.append((s.name, str(e).splitlines()[0] if str(e) else "assert"))
    assert not failed, failed


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("S", [15, 31])
def test_every_footprint_position_of_a_tile(ctx, oracle, S, geom):
    """C 6: one visibility at every cell of a window two cells larger than the tile: every footprint position a tile can
    hold, its corners included.  Under the default geometry the tile is the one the library reports."""
    opts = geometry(geom, S)
    if geom == "default":
        check_exact(ctx, oracle, S, "one_run_1", opts)
        tile = (ctx.get_option("last_tile_x"), ctx.get_option("last_tile_y"))
        assert tile == (K.SMALL_TILE,) * 2
    else:
        tile = K.PROD_TILE[S]
    check_exact(ctx, oracle, S, f"window_{tile[0]}x{tile[1]}", opts, tile=tile)


def aw_form_of(s, seed, S):
    """a structured stream as an aw call: plane p of its W becomes (wbin, a1, a2) = (p % 2, p // 2 % 2, p // 4), so
    equal slices stay equal kernels and different ones different; wbin = W stays out of range"""
    rng = np.random.default_rng(seed)
    W, A = 2, max(2, -(-s.W // 4))
    wb = np.where(s.wb >= s.W, W, s.wb % 2)
    a1, a2 = np.where(s.wb >= s.W, 0, s.wb // 2 % 2), np.where(s.wb >= s.W, 0, s.wb // 4)
    wk = rng.normal(size=(W, s.Q, s.Q, S, S)) + 1j * rng.normal(size=(W, s.Q, s.Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    n = len(s.u)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    G = rng.normal(size=(K.HC, K.WDC)) + 1j * rng.normal(size=(K.HC, K.WDC))
    return wk, ak, s.u, s.v, wb.astype(np.int64), a1.astype(np.int64), a2.astype(np.int64), vis, G


@functools.lru_cache(maxsize=None)
def aw_stream_refs(S, name):
    s = STREAMS[name]
    case = aw_form_of(s, S * 100 + len(name), S)
    return s, case, aw_refs(case[0], case[1], K.HC, K.WDC, *case[2:])


@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("S", K.AW_CLASS_SUPPORTS)
def test_structured_streams_aw(ctx, S, geom):
    """C 1 - 5 in the aw form (the sorted list carries the kernel's index, the sorter stages values or origins).  The
    w-groups of stream 7 do not exist there."""
    opts = geometry(geom, S)
    failed = []
    for name in [x for x in STREAMS if not x.startswith("wgroups")]:
        s, case, (ref, dref, _) = aw_stream_refs(S, name)
        with options(ctx, **{**opts, **s.opts}):
            try:
                g, d = aw_calls(ctx, K.HC, K.WDC, *case)
                assert ctx.last_dropped() == (1 if s.ndrop else 0)
                assert rel(g, ref) < TOL and np.isfinite(d).all() and rel(d, dref) < TOL
                assert not d[dref == 0].any() and (dref == 0).sum() == s.ndrop
            except AssertionError as e:
                failed.append((name, str(e).splitlines()[0] if str(e) else "assert"))
    assert not failed, failed
