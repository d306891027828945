"""Reprojection and mosaicking on the device (gridhip_mosaic[_dev], gridhip_reproject[_dev]) against the numpy restatement
tests/mosaic_ref.py.  EVERYTHING a call writes - the image, the weight sums, the eight stats - is compared bit for bit, in
the host form and in the _dev form: every cell's sums belong to one thread and fp64 multiply, add, divide, sqrt and floor
are correctly rounded on both sides, so there is no tolerance to state.  The shapes are the smallest at which each path
can go wrong: facets smaller than a footprint, destinations of one cell, one short of, equal to and one past a tile,
several tiles, lists of one, two and five facets, and the cull where the map bends most.  Only the end-to-end test is a
statement about positions."""
import ctypes as C

import numpy as np
import pytest

import mosaic_ref as M

pytestmark = pytest.mark.gpu

f64 = np.float64
EINVAL, EUNSUPPORTED = -1, -5
KINDS = ("nearest", "bilinear", "cubic")
CENTRES = [(0.0, 0.0), (0.03, -0.02), (-0.04, 0.03), (0.05, 0.05), (-0.02, -0.05)]


def dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def rotations(centres):
    import gridhip
    return np.array([gridhip.rotation_to(l0, m0).ravel() for l0, m0 in centres])


def check(ctx, what, facets, theta_s, R, theta_d, Nd, kind, weights=None, forms=("host", "dev"), **kw):
    """the host form and the _dev form against the restatement: out, wsum and the stats, bit for bit; returns the reference"""
    want = M.mosaic(facets, theta_s, R, theta_d, Nd, kind, weights=weights, **kw)
    for form in forms:
        if form == "host":
            got = ctx.mosaic(facets, theta_s, R, theta_d, Nd, kind, weights=weights, wsum=True, stats=True, **kw)
        else:
            got = [host(a) for a in ctx.mosaic(dev(facets), theta_s, dev(R), theta_d, Nd, kind, weights=dev(weights), wsum=True,
                                               stats=True, **kw)]
        for name, a, b in zip(("out", "wsum", "stats"), got, want):
            assert M.same_bits(a, b), f"{what} [{form}] {name}: {int((a != b).sum())} values differ"
    return want


# ---- every kind at the edge shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_edge_shapes(ctx, kind):
    """Ns below, at and above a footprint; Nd about the 16-cell tile; 1, 2 and 5 overlapping facets; a feathered and a hard
    window.  The destination's cell is a quarter of the facets', so that several destination cells share a tap."""
    rng = np.random.default_rng(KINDS.index(kind))
    R5 = rotations(CENTRES)
    covered = 0
    for Ns in (1, 3, 4, 5, 17):
        fac = rng.normal(size=(5, Ns, Ns))
        for Nd in (1, 15, 16, 17, 33):
            for F in (1, 2, 5):
                for window in ((Ns / 4, Ns / 2), (Ns / 2.5, Ns / 2.5), None):
                    want = check(ctx, f"Ns {Ns} Nd {Nd} F {F} window {window}", fac[:F], 0.15, R5[:F], 0.2, Nd, kind, window=window)
                    covered += int(want[2][0])
                    if Ns >= 5 and Nd >= 15:  # (where the cubic has more than one place to stand)
                        assert want[2][0] > 0 and (F == 1 or want[2][5] >= 2)  # something is covered, and by several
    assert covered > 0


def test_reproject_is_the_one_facet_case(ctx):
    rng = np.random.default_rng(3)
    img, R = rng.normal(size=(17, 17)), rotations([(0.03, -0.02)])[0].reshape(3, 3)
    for kind in KINDS:
        want = M.reproject(img, 0.15, R, 0.2, 33, kind, window=(5.0, 8.0), blank=-3.0)
        assert M.same_bits(ctx.reproject(img, 0.15, R, 0.2, 33, kind, window=(5.0, 8.0), blank=-3.0), want)
        out = dev(np.zeros((33, 33)))
        assert ctx.reproject(dev(img), 0.15, R, 0.2, 33, kind, window=(5.0, 8.0), blank=-3.0, out=out) is out  # (a host R is uploaded)
        assert M.same_bits(host(out), want)
    # the way back: R^T takes the destination's plane to the facet's
    back = ctx.reproject(np.ones((33, 33)), 0.2, R.T, 0.15, 17, "bilinear")
    assert np.nanmax(np.abs(back - 1.0)) <= 4 * np.finfo(f64).eps and np.isfinite(back).sum() > 200


# ---- the cull ---------------------------------------------------------------------------------------------------------------
def with_option(ctx, key, value):
    class _Scope:
        def __enter__(self):
            ctx.set_option(key, value)

        def __exit__(self, *exc):
            ctx.set_option(key, 0)
    return _Scope()


@pytest.mark.parametrize("kind", KINDS)
def test_the_cull_where_the_map_is_least_affine(ctx, kind):
    """theta_d = 1.6: the destination's corners lie at r = 1.13, beyond the horizon, and the two facets sit where n is
    0.74 and 0.67.  The culled walk, the walk over all facets (option "mosaic_cull" = 1) and the restatement, which has
    no cull, give the same bits; a third facet that reaches nothing changes none of them."""
    rng = np.random.default_rng(11)
    Ns, Nd = 32, 48
    R = rotations([(0.6, 0.3), (-0.5, -0.55), (0.0, 0.0)])
    fac = rng.normal(size=(3, Ns, Ns))
    for theta_s, window in ((0.5, (10.0, 16.0)), (0.9, None), (0.02, (3.0, 3.0))):
        want = check(ctx, f"theta_s {theta_s}", fac, theta_s, R, 1.6, Nd, kind, window=window)
        with with_option(ctx, "mosaic_cull", 1):
            check(ctx, f"theta_s {theta_s}, no cull", fac, theta_s, R, 1.6, Nd, kind, window=window, forms=("dev",))
        assert want[2][2] == 3 and (theta_s == 0.02 or want[2][0] > 0)
    two = check(ctx, "two facets", fac[:2], 0.5, R[:2], 1.6, Nd, kind, window=(10.0, 16.0))
    none = rotations([(0.6, 0.3), (-0.5, -0.55), (0.0, 0.0)])
    none[2] = rotations([(-0.7, 0.68)])[0]  # (n0 = 0.22: its window lies outside the destination's field altogether)
    three = check(ctx, "a facet that covers nothing", fac, 0.05, none, 0.4, Nd, kind, window=(10.0, 16.0))
    assert three[2][0] == 0 and three[2][2] == 3 and two[2][0] > 0


def test_more_facets_than_one_pass_of_the_cull(ctx):
    """300 facets: the work-group's 256 threads test them in two passes, and the list keeps the order across the passes -
    with 1 - 9 of them on a cell, any other order would change the sums' bits.  Valid and refused facets alternate in places."""
    rng = np.random.default_rng(19)
    F, Ns, Nd = 300, 9, 40
    R = rotations(rng.uniform(-0.1, 0.1, size=(F, 2)))
    R[rng.integers(0, F, 12), 8] = -1.0
    fac = rng.normal(size=(F, Ns, Ns))
    for kind in ("bilinear", "cubic"):
        want = check(ctx, kind, fac, 0.04, R, 0.25, Nd, kind, window=(2.0, 4.5), forms=("dev",))
        with with_option(ctx, "mosaic_cull", 1):
            check(ctx, f"{kind}, no cull", fac, 0.04, R, 0.25, Nd, kind, window=(2.0, 4.5), forms=("dev",))
        assert want[2][3] >= 10 and want[2][2] + want[2][3] == F and want[2][5] >= 3 and want[2][0] > Nd * Nd // 2


def test_a_facet_that_covers_exactly_one_cell_of_a_tile(ctx):
    """The facet's centre is the direction of one destination cell and the hard window keeps |fx - Ns/2| <= 0.4 at equal
    cell sizes: that cell alone.  At a tile's first and last cell, and in its middle, with and without a facet beside it."""
    rng = np.random.default_rng(12)
    Ns, Nd, theta_d = 8, 48, 0.3
    theta_s = theta_d * Ns / Nd
    lc = M.cell_coords(Nd, theta_d)
    fac = rng.normal(size=(2, Ns, Ns))
    for x, y in ((16, 31), (31, 16), (0, 0), (47, 47), (24, 40)):
        R = rotations([(lc[x], lc[y]), (0.0, 0.0)])
        out, wsum, st = check(ctx, f"cell ({x}, {y})", fac[:1], theta_s, R[:1], theta_d, Nd, "nearest", window=(0.4, 0.4), blank=0.0)
        assert st[0] == 1 and wsum[y, x] == 1.0 and out[y, x] == fac[0, Ns // 2, Ns // 2]
        out, wsum, st = check(ctx, f"cell ({x}, {y}) beside a facet", fac, theta_s, R, theta_d, Nd, "nearest", window=(0.4, 0.4))
        assert st[0] == 2 and wsum[y, x] == 1.0 and wsum[Nd // 2, Nd // 2] == 1.0


def test_the_horizon(ctx):
    """theta_d = 2.2: the corners have r2 >= 1 and are blank, whatever lies there in a facet's plane"""
    rng = np.random.default_rng(13)
    Nd = 33
    R = rotations([(0.0, 0.0), (0.5, 0.4)])
    fac = rng.normal(size=(2, 17, 17))
    for kind in KINDS:
        out, wsum, st = check(ctx, kind, fac, 2.2, R, 2.2, Nd, kind, blank=-9.0)
        lc = M.cell_coords(Nd, 2.2)
        l, m = np.meshgrid(lc, lc)
        beyond = ~(l * l + m * m < 1.0)
        assert beyond[0, 0] and beyond[0, -1] and beyond[-1, 0] and beyond[-1, -1]
        assert np.all(out[beyond] == -9.0) and np.all(wsum[beyond] == 0.0) and st[0] > 0 and st[1] >= beyond.sum()


# ---- what is left out ---------------------------------------------------------------------------------------------------------
def test_refused_rotations_are_counted_and_left_out_on_the_device(ctx):
    """the _dev form takes R from device memory: a facet with R22 <= 0, one with a NaN entry and one that is no rotation
    contribute nothing and are counted - where the host-array R of the binding is refused before the call"""
    rng = np.random.default_rng(14)
    R = rotations(CENTRES)
    R[1] = np.diag([1.0, -1.0, -1.0]).ravel()
    R[2, 3] = np.nan
    R[4, 0] *= 1.0 + 1e-6
    fac = rng.normal(size=(5, 17, 17))
    for kind in KINDS:
        out, wsum, st = check(ctx, kind, fac, 0.15, R, 0.2, 33, kind, window=(4.0, 8.0), forms=("dev",))
        assert st[2] == 2 and st[3] == 3 and st[5] == 2
        good = M.mosaic(fac[[0, 3]], 0.15, R[[0, 3]], 0.2, 33, kind, window=(4.0, 8.0))
        assert M.same_bits(out, good[0]) and M.same_bits(wsum, good[1])
    with pytest.raises(ValueError):
        ctx.mosaic(fac, 0.15, R, 0.2, 33)
    with pytest.raises(ValueError):
        ctx.mosaic(dev(fac), 0.15, R, 0.2, 33)  # (a host R beside cuda facets is checked on the host too)
    # the C ABI's host form has the same rule as its _dev form: counted, not refused
    out, st = np.zeros((33, 33)), np.zeros(8)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    rc = ctx._lib.gridhip_mosaic(ctx._h, 5, 17, 0.15, p(fac), None, p(R), 1, 4.0, 8.0, 1, 0.0, float("nan"), 33, 0.2, p(out), None, p(st))
    want = M.mosaic(fac, 0.15, R, 0.2, 33, "bilinear", window=(4.0, 8.0))
    assert rc == 0 and M.same_bits(out, want[0]) and M.same_bits(st, want[2])


@pytest.mark.parametrize("kind", KINDS)
def test_weights_and_cells_that_are_not_finite(ctx, kind):
    """a weight image with zeros, negatives, NaN and Inf; NaN and Inf source cells under good weights (left out, counted),
    under bad ones and outside the window (never seen); normalize on and off; wmin above some cells' den"""
    rng = np.random.default_rng(15)
    F, Ns, Nd = 3, 17, 33
    R = rotations(CENTRES[:F])
    fac = rng.normal(size=(F, Ns, Ns))
    wt = rng.uniform(0.5, 2.0, size=(F, Ns, Ns))
    wt[0, 2:6, 2:9] = 0.0
    wt[0, 6:9, 2:9] = -1.0
    wt[1, 10:13, 3:12] = np.nan
    wt[2, 4, 4] = np.inf
    fac[0, 3:8, 4:7] = np.nan      # under zero and negative weights
    fac[1, 8, 8] = np.inf          # inside the window, under a good weight
    fac[1, 11, 5] = -np.inf        # under a NaN weight
    fac[2, 0, :] = np.nan          # outside the window
    fac[2, 9, 3] = np.nan
    window = (4.0, 7.5)
    for weights in (wt, None):
        for normalize, wmin in ((True, 0.0), (False, 0.0), (True, 0.75), (False, 2.0)):
            out, wsum, st = check(ctx, f"weights {weights is not None} normalize {normalize} wmin {wmin}", fac, 0.15, R, 0.2, Nd, kind,
                                  weights=weights, window=window, normalize=normalize, wmin=wmin, blank=-5.0)
            assert np.isfinite(out).all() and st[4] > 0 and st[0] > 0 and st[0] + st[1] == Nd * Nd
            assert np.all(wsum[out == -5.0] == 0.0) and np.all(wsum[wsum > 0] > wmin)
    few = M.mosaic(fac, 0.15, R, 0.2, Nd, kind, weights=wt, window=window, wmin=0.75)[2][0]
    assert few < M.mosaic(fac, 0.15, R, 0.2, Nd, kind, weights=wt, window=window)[2][0]  # (wmin did blank some cells)


# ---- determinism, capture, refusals --------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(ctx):
    import gridhip
    rng = np.random.default_rng(16)
    centres, R, theta_f, window = gridhip.facet_grid(0.3, 3, 0.3, 40)
    fac, wt = dev(rng.normal(size=(9, 40, 40))), dev(rng.uniform(0.1, 1.0, size=(9, 40, 40)))
    dR = dev(R)
    runs = [[host(a) for a in ctx.mosaic(fac, theta_f, dR, 0.3, 100, "cubic", weights=wt, window=window, wsum=True, stats=True)]
            for _ in range(2)]
    for a, b in zip(*runs):
        assert M.same_bits(a, b)
    want = M.mosaic(host(fac), theta_f, R, 0.3, 100, "cubic", weights=host(wt), window=window)
    for a, b in zip(runs[0], want):
        assert M.same_bits(a, b)
    assert want[2][1] == 0 and want[2][5] == 4  # no gap anywhere, and four facets meet at the inner corners


def test_a_captured_mosaic_replays_on_changed_facets(ctx):
    import torch
    import gridhip
    rng = np.random.default_rng(17)
    centres, R, theta_f, window = gridhip.facet_grid(0.2, 2, 0.3, 24)
    data = [rng.normal(size=(4, 24, 24)) for _ in range(2)]
    fac, dR = dev(data[0]), dev(R)
    out = dev(np.zeros((50, 50)))

    def step():
        return ctx.mosaic(fac, theta_f, dR, 0.2, 50, "cubic", window=window, wsum=True, stats=True, out=out)

    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        res = step()
    torch.cuda.synchronize()
    for d in (data[1], data[0]):
        fac.copy_(dev(d))
        for a in res:
            a.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("out", "wsum", "stats"), res, M.mosaic(d, theta_f, R, 0.2, 50, "cubic", window=window)):
            assert M.same_bits(host(a), b), name


def test_refusals(ctx):
    """every rule of the header that needs a context; nothing is touched by a refused call"""
    import torch
    import gridhip
    F, Ns, Nd = 2, 8, 16
    fac, wt, R = dev(np.full((F, Ns, Ns), 2.0)), dev(np.full((F, Ns, Ns), 3.0)), dev(rotations(CENTRES[:F]))
    out, ws, st = dev(np.full((Nd, Nd), 5.0)), dev(np.full((Nd, Nd), 6.0)), dev(np.full(8, 7.0))
    lib, h, nan = ctx._lib, ctx._h, float("nan")
    p = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(F=F, Ns=Ns, ths=0.1, fac=fac, wt=wt, R=R, kind=3, inner=2.0, outer=4.0, wmin=0.0, Nd=Nd, thd=0.2, out=out, ws=ws,
             st=st, off=0):
        ctx._use_torch_stream()
        return lib.gridhip_mosaic_dev(h, F, Ns, ths, p(fac), p(wt), p(R), kind, inner, outer, 1, wmin, nan, Nd, thd, p(out, off),
                                      p(ws), p(st))
    assert call() == 0
    torch.cuda.synchronize()
    out.fill_(5.0), ws.fill_(6.0), st.fill_(7.0)
    for bad in (dict(fac=None), dict(R=None), dict(out=None), dict(F=0), dict(Ns=0), dict(Nd=0), dict(ths=0.0), dict(ths=-0.1),
                dict(ths=nan), dict(thd=float("inf")), dict(thd=0.0), dict(kind=2), dict(kind=-1), dict(kind=4), dict(inner=-1.0),
                dict(inner=3.0, outer=2.0), dict(outer=float("inf")), dict(inner=nan), dict(wmin=-1.0), dict(wmin=nan),
                dict(out=fac), dict(out=wt), dict(ws=fac), dict(ws=out), dict(st=R), dict(out=R), dict(out=ws, off=8),
                dict(out=fac, off=8 * Ns * Ns)):  # (out inside the second facet)
        assert call(**bad) == EINVAL, bad
        assert ctx._error(EINVAL)
    big = dev(np.zeros((4097, 1, 1)))
    assert call(F=4097, Ns=1, fac=big, wt=None, R=dev(np.tile(np.eye(3).ravel(), (4097, 1)))) == EUNSUPPORTED
    assert call(Ns=32769) == EUNSUPPORTED and call(Nd=32769) == EUNSUPPORTED  # (judged on the sizes: nothing is read)
    assert lib.gridhip_reproject_dev(h, Ns, 0.1, p(fac), p(R), 3, 2.0, 4.0, nan, Nd, 0.2, p(fac)) == EINVAL
    torch.cuda.synchronize()
    for t, val in ((fac, 2.0), (wt, 3.0), (out, 5.0), (ws, 6.0), (st, 7.0)):
        assert bool((t == val).all())
    with pytest.raises(gridhip.GridHipError) as e:  # through the binding: out is a view of the facets
        ctx.mosaic(fac, 0.1, R, 0.2, Ns, out=fac[0])
    assert e.value.code == EINVAL
    with pytest.raises(gridhip.GridHipError) as e:
        ctx.reproject(fac[0], 0.1, R[0], 0.2, Ns, out=fac[0])
    assert e.value.code == EINVAL
    hfac = host(fac)
    with pytest.raises(gridhip.GridHipError) as e:  # and the host form
        ctx.mosaic(hfac, 0.1, host(R), 0.2, Ns, out=hfac[1])
    assert e.value.code == EINVAL and np.all(hfac == 2.0)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_facets_imaged_about_their_own_centres_come_back_onto_one_plane(ctx):
    """Three point sources through dft_predict on 4000 baselines; facet_grid's 2 x 2 facets of 64^2 cells, each made by
    phase_shift(R_f) and imaged about its own centre; the mosaic on 128^2 cells.  One source sits at a facet's centre, one
    inside another facet and one on the seam where all four facets are feathered together.  The three brightest local
    maxima lie within one cell of the sources' cells: a statement about positions, with one cell for the dirty beam and
    the interpolation."""
    import gridhip
    rng = np.random.default_rng(18)
    theta, Nd, Nf, lam, n = 0.16, 128, 64, 640, 4000
    centres, R, theta_f, window = gridhip.facet_grid(theta, 2, 0.25, Nf)
    assert abs(theta_f - 0.1) < 1e-15 and ctx.image_size(theta_f, lam) == Nf
    cells = [(32, 32), (90, 41), (61, 68)]  # (x, y); facet 0's centre is (32, 32)
    flux = [1.0, 0.8, 0.6]
    lc = M.cell_coords(Nd, theta)
    assert abs(lc[32] - centres[0, 0]) < 1e-15
    comps = gridhip.components([lc[x] for x, _ in cells], [lc[y] for _, y in cells], flux)
    u, v = np.clip(rng.normal(0, 90.0, (2, n)), -280, 280)
    uvw = dev(np.stack([u, v, np.zeros(n)], axis=1))
    vis = ctx.dft_predict(uvw, dev(comps))
    images = []
    for f in range(4):
        vis_f, uvw_f = ctx.phase_shift(uvw, vis, R[f].reshape(3, 3))
        im = ctx.imager(theta_f, lam, uvw_f, ("simple",), weighting="natural")
        images.append(im.cycle(vis_f).clone())
        im.close()
    import torch
    out, stats = ctx.mosaic(torch.stack(images), theta_f, dev(R), theta, Nd, "cubic", window=window, stats=True)
    out, stats = host(out), host(stats)
    assert stats[1] == 0 and stats[2] == 4 and stats[4] == 0 and stats[5] == 4 and np.isfinite(out).all()
    inner = out[1:-1, 1:-1]
    peak = np.ones_like(inner, dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                peak &= inner > out[1 + dy:Nd - 1 + dy, 1 + dx:Nd - 1 + dx]
    ys, xs = np.nonzero(peak)
    top = np.argsort(inner[ys, xs])[-3:][::-1]
    found = [(int(xs[k]) + 1, int(ys[k]) + 1) for k in top]
    print("sources at", cells, "maxima at", found, "values", [float(out[y, x]) for x, y in found])
    for (x, y), (fx, fy) in zip(cells, found):  # (in order of flux)
        assert abs(x - fx) <= 1 and abs(y - fy) <= 1, (cells, found)
