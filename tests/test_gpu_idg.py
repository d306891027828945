"""Image-domain layers on the GPU (qpx = 0 in the w-stacking entry points; ("idg", ...) in Context.do_imaging, predict,
wstack and imager) against the numpy restatement tests/idg_ref.py.

Tolerances are derived, not measured.  An uncorrected image cell is a sum of n terms of size |vis_k| / N^2, each with a few
roundings and a phase below 100 turns, so per cell |got - ref| <= 1e-12 x C[y][x] x sum_k |vis_k| / N^2 (exactly 0 outside
the trusted region, where C is 0), and per visibility |got - ref| <= 1e-12 x sum |C x model|.  do_imaging and an imager
divide by pmax, whose own relative error is of the same 1e-12: their cells get 2e-12 x C x (2 sum_k |wt_k vis_k| / N^2) / pmax.

Shapes: N = 64 and 65 (theta 0.1, lam 640 and 650), 300 to 600 visibilities, wstep 100, |w| <= 1500."""
import ctypes as C

import numpy as np
import pytest

import idg_ref as I
import wstack_ref as W
from oracle import gridref_np as R

pytestmark = pytest.mark.gpu

THETA, WSTEP = 0.1, 100
LAMS = {64: 640, 65: 650}
EPS = 1e-12


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def bits(z):
    z = np.ascontiguousarray(z)
    return z.view(np.uint64).reshape(z.shape + (-1,))


def fn(sk, M):
    return ("idg", dict(wstep=WSTEP, planes=M, subgrid=sk[0], margin=sk[1]))


def within(got, ref, tol, what):
    """|got - ref| <= tol element by element; prints the largest ratio"""
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, d / tol, np.where(d > 0, np.inf, 0.0)).max() if d.size else 0.0
    print(f"  {what}: {ratio:.3g} of the bound")
    assert np.isfinite(got).all() and ratio <= 1.0, f"{what}: {ratio} of the bound"


def image_tol(N, K, amp):
    return EPS * I.correction(N, K) * amp


def predict_tol(N, K, model):
    return EPS * np.abs(I.correction(N, K) * model).sum()


_cases = {}


def case(N, sk, M, n=400, span=0.45, seed=3):
    key = (N, sk, M, n, span, seed)
    if key not in _cases:
        lam = LAMS[N]
        rng = np.random.default_rng(seed)
        u, v = rng.uniform(-span * lam, span * lam, n), rng.uniform(-span * lam, span * lam, n)
        w = rng.uniform(-1500, 1500, n)
        vis = rng.normal(size=n) + 1j * rng.normal(size=n)
        model = rng.normal(size=(N, N))
        ref = I.Stack(THETA, lam, u, v, w, WSTEP, M, *sk)
        _cases[key] = dict(N=N, lam=lam, sk=sk, M=M, u=u, v=v, w=w, vis=vis, model=model, ref=ref, image=ref.image(vis),
                           pred=ref.predict(model), imaging=I.do_imaging(THETA, lam, u, v, w, vis, WSTEP, M, *sk))
    return _cases[key]


def dev3(c):
    return tuple(to_dev(c[k]) for k in "uvw")


# ---- 1: parity with the restatement, every form ---------------------------------------------------------------------------------
PARITY = [(64, (16, 4), 4), (65, (16, 8), 1), (64, (24, 12), 4), (65, (32, 16), 4), (64, (32, 16), 1)]


def handle_parity(ctx, c):
    import torch
    N, sk, ref = c["N"], c["sk"], c["ref"]
    ws = ctx.wstack(THETA, c["lam"], dev3(c), fn(sk, c["M"]))
    assert (ws.layers, ws.occupied, ws.pmin, ws.dropped) == (ref.lay["L"], len(ref.occupied), ref.lay["pmin"], ref.dropped)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    it, pt = image_tol(N, sk[1], np.abs(c["vis"]).sum() / N ** 2), predict_tol(N, sk[1], c["model"])
    within(host(ws.image(dvis)), c["image"], it, "handle image")
    pred = host(ws.predict(dmodel))
    within(pred, c["pred"], pt, "handle predict")
    assert np.array_equal(bits(host(ws.predict(dmodel))), bits(pred))  # the same bits every run
    within(host(ws.predict(dmodel, vis_sub=dvis)), c["vis"] - c["pred"], pt, "residual")
    buf = dvis.clone()
    assert ws.predict(dmodel, vis_sub=buf, out=buf) is buf
    within(host(buf), c["vis"] - c["pred"], pt, "residual in place")
    within(host(ws.image(dvis)), c["image"], it, "image again")  # the grid is clear again
    # a second call takes no memory
    out, img = torch.zeros_like(dvis), ws.image(dvis)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    ws.image(dvis, out=img), ws.predict(dmodel, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    ws.close()
    return pred


def calls_parity(ctx, c):
    import torch
    N, sk, lam, f = c["N"], c["sk"], c["lam"], fn(c["sk"], c["M"])
    r_img, r_psf, r_pmax = c["imaging"]
    u1, v1, w1, vis1 = R.mirror_uvw(c["u"], c["v"], c["w"], c["vis"])
    wt = np.abs(R.doweight(N, u1 / np.float64(lam), v1 / np.float64(lam), np.ones(len(u1), dtype=np.complex128)))
    it = 2 * image_tol(N, sk[1], 2 * (wt * np.abs(vis1)).sum() / N ** 2 / r_pmax)
    ipsf = 2 * image_tol(N, sk[1], 2 * wt.sum() / N ** 2 / r_pmax)
    pt = predict_tol(N, sk[1], c["model"])
    uvw = np.stack([c["u"], c["v"], c["w"]], axis=1)  # the (n, 3) matrix: stride 3
    img, psf, pmax = ctx.do_imaging(THETA, lam, uvw, None, None, None, None, c["vis"], f)
    dargs = (THETA, lam, dev3(c), None, None, None, None, to_dev(c["vis"]), f)
    dimg, dpsf, dpmax = ctx.do_imaging(*dargs)
    for tag, a, b, p in (("host", img, psf, pmax), ("device", host(dimg), host(dpsf), dpmax)):
        within(a, r_img, it, f"do_imaging image ({tag})")
        within(b, r_psf, ipsf, f"do_imaging psf ({tag})")
        assert abs(p - r_pmax) <= EPS * 2 * wt.sum() / N ** 2, tag
    pred = ctx.predict(THETA, lam, uvw, c["model"], f)
    dpred = ctx.predict(THETA, lam, to_dev(uvw), to_dev(c["model"]), f)
    within(pred, c["pred"], pt, "predict (host)")
    assert np.array_equal(bits(host(dpred)), bits(pred))  # host and device forms: bit for bit
    sub = c["vis"].copy()
    assert ctx.predict(THETA, lam, (c["u"], c["v"], c["w"]), c["model"], f, vis_sub=sub, out=sub) is sub
    within(sub, c["vis"] - c["pred"], pt, "vis_sub in place (host)")
    dsub = to_dev(c["vis"])
    within(host(ctx.predict(THETA, lam, dev3(c), to_dev(c["model"]), f, vis_sub=dsub)), c["vis"] - c["pred"], pt, "vis_sub (device)")
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    ctx.do_imaging(*dargs), ctx.predict(THETA, lam, dev3(c), to_dev(c["model"]), f, vis_sub=dsub, out=dsub)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    return pred


@pytest.mark.parametrize("N,sk,M", PARITY, ids=str)
def test_parity_with_the_restatement(ctx, N, sk, M):
    c = case(N, sk, M)
    print(f"N={N} {sk} M={M}")
    a = handle_parity(ctx, c)
    b = calls_parity(ctx, c)
    assert np.array_equal(bits(a), bits(b))  # a handle's prediction and the one-call form's
    assert ctx.get_option("errors") == 0


# ---- 2: edges -----------------------------------------------------------------------------------------------------------------------
def check_stream(ctx, N, u, v, w, sk, M, seed=5, what=""):
    """a handle's image and predict of a stream against the restatement, the dropped count and the dropped predictions"""
    lam, n = LAMS[N], len(u)
    rng = np.random.default_rng(seed)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    ref = I.Stack(THETA, lam, u, v, w, WSTEP, M, *sk)
    print(f"{what}: N={N} {sk} M={M} n={n} dropped {ref.dropped} layers {ref.lay['L']} occupied {len(ref.occupied)}")
    ws = ctx.wstack(THETA, lam, tuple(to_dev(np.asarray(x, dtype=np.float64)) for x in (u, v, w)), fn(sk, M))
    assert (ws.layers, ws.occupied, ws.dropped) == (ref.lay["L"], len(ref.occupied), ref.dropped)
    assert ctx.last_dropped() == ref.dropped
    dvis, dmodel = to_dev(vis), to_dev(model)
    within(host(ws.image(dvis)), ref.image(vis), image_tol(N, sk[1], np.abs(vis).sum() / N ** 2), "image")
    pred = host(ws.predict(dmodel))
    within(pred, ref.predict(model), predict_tol(N, sk[1], model), "predict")
    assert np.all(bits(pred)[~ref.keep] == 0)  # exactly +0
    res = host(ws.predict(dmodel, vis_sub=dvis))
    assert np.array_equal(bits(res)[~ref.keep], bits(vis)[~ref.keep])
    ws.close()
    assert ctx.get_option("errors") == 0
    return ref


def cells(N, x):
    """u (or v) whose cell coordinate N (u / lam) + N div 2 is exactly x, for x with few bits: N = 64, lam = 640"""
    assert N == 64
    u = (np.asarray(x, dtype=np.float64) - 32.0) * 10.0
    assert np.array_equal(64.0 * (u / 640.0) + 32.0, np.asarray(x, dtype=np.float64))
    return u


@pytest.mark.parametrize("sk", [(16, 8), (24, 12)], ids=str)
def test_tile_boundaries_and_grid_borders(ctx, sk):
    T = sk[0] - sk[1]
    eps = 2.0 ** -40
    on = np.arange(0, 64, T, dtype=np.float64)
    xs = np.concatenate([on, on[1:] - eps, [64 - eps, 63.0, 0.0, 0.5]])  # on and just below every boundary; the borders
    rng = np.random.default_rng(2)
    x, y = np.concatenate([xs, rng.permutation(xs), xs]), np.concatenate([xs, xs, rng.permutation(xs)])
    w = rng.uniform(-300, 300, len(x))
    ref = check_stream(ctx, 64, cells(64, x), cells(64, y), w, sk, 4, what="boundaries and borders")
    assert ref.dropped == 0 and ref.ox.min() < 0 and ref.ox.max() + sk[0] > 64  # subgrids clipped on either side
    assert np.sum(ref.a == -T / 2) >= len(on)


def test_dropped_visibilities(ctx):
    """outside the grid on either side and axis, NaN in u, v and w, an infinite w: dropped, counted, predicted exactly 0"""
    eps = 2.0 ** -40
    rng = np.random.default_rng(4)
    n = 300
    x, y = rng.uniform(0, 64, n), rng.uniform(0, 64, n)
    w = rng.uniform(-1500, 1500, n)
    x[:6] = [64.0, -eps, 70.0, np.nan, 5.0, 64 - eps]
    y[6:10] = [64.0, -1.0, np.nan, 0.0]
    w[10:13] = [np.nan, np.inf, -np.inf]
    u, v = (x - 32.0) * 10.0, (y - 32.0) * 10.0
    ref = check_stream(ctx, 64, u, v, w, (16, 8), 4, what="dropped")
    assert ref.dropped == 4 + 3 + 3 and ref.keep[4] and ref.keep[5] and ref.keep[9]
    # odd N, T = 12 does not divide it
    lam = 650
    u, v = rng.uniform(-0.52 * lam, 0.52 * lam, n), rng.uniform(-0.52 * lam, 0.52 * lam, n)
    ref = check_stream(ctx, 65, u, v, w, (16, 4), 1, what="dropped, N = 65")
    assert ref.dropped > 13


def test_small_and_empty_streams(ctx):
    import torch
    one = check_stream(ctx, 64, [37.0], [-110.0], [420.0], (24, 12), 4, what="one visibility")
    assert one.dropped == 0
    # an empty layer between occupied ones: planes 0, 1 and 9 with M = 3 -> layers 0 and 3 of 4
    rng = np.random.default_rng(6)
    n = 60
    w = np.where(np.arange(n) % 2 == 0, rng.uniform(0, 140, n), rng.uniform(860, 940, n))
    gap = check_stream(ctx, 65, rng.uniform(-250, 250, n), rng.uniform(-250, 250, n), w, (16, 8), 3, what="an empty layer")
    assert gap.lay["L"] == 4 and gap.occupied == [0, 3]
    # n = 0: a zero image, no prediction
    e = torch.zeros(0, dtype=torch.float64, device="cuda:0")
    ws = ctx.wstack(THETA, 640, (e, e, e), fn((16, 8), 4))
    img = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
    ws.image(torch.zeros(0, dtype=torch.complex128, device="cuda:0"), out=img)
    assert not bool(img.any()) and ws.predict(to_dev(np.ones((64, 64)))).shape == (0,) and (ws.layers, ws.dropped) == (0, 0)
    ws.close()
    img, psf, pmax = ctx.do_imaging(THETA, 640, (np.zeros(0), np.zeros(0), np.zeros(0)), None, None, None, None,
                                    np.zeros(0, dtype=np.complex128), fn((16, 8), 4))
    assert img.shape == (64, 64) and ctx.predict(THETA, 640, (np.zeros(0),) * 3, np.ones((64, 64)), fn((16, 8), 4)).shape == (0,)
    # every visibility dropped: a zero image, zero predictions
    ref = check_stream(ctx, 64, [400.0, -500.0], [0.0, 0.0], [0.0, 100.0], (16, 8), 4, what="all dropped")
    assert ref.dropped == 2
    assert ctx.get_option("errors") == 0


def test_one_tile_either_side_of_the_chunk_and_the_split(ctx):
    chunk, split = ctx.get_option("idg_chunk"), ctx.get_option("idg_split")
    assert chunk >= 2 and split > chunk
    for sk in ((16, 8), (24, 12), (32, 16)):
        T = sk[0] - sk[1]
        lo = T * (24 // T)  # one tile near the centre: cells [lo, lo + T)
        for n in (chunk - 1, chunk, chunk + 1, split + 1) if sk == (16, 8) else (chunk + 1, split + 1):
            rng = np.random.default_rng(n)
            x, y = rng.uniform(lo, lo + T, n), rng.uniform(lo, lo + T, n)
            x[0], y[0] = lo, lo
            ref = check_stream(ctx, 64, (x - 32.0) * 10.0, (y - 32.0) * 10.0, rng.uniform(-40, 40, n), sk, 4, what=f"one tile of {n}")
            assert len(set(zip(ref.tx.tolist(), ref.ty.tolist()))) == 1 and len(ref.occupied) == 1 and ref.dropped == 0


def test_two_tiles_whose_subgrids_overlap(ctx):
    rng = np.random.default_rng(8)
    n = 40
    x = np.where(np.arange(n) % 2 == 0, rng.uniform(24, 32, n), rng.uniform(32, 40, n))  # tiles 3 and 4 of T = 8
    y = rng.uniform(24, 32, n)
    ref = check_stream(ctx, 64, (x - 32.0) * 10.0, (y - 32.0) * 10.0, np.zeros(n), (16, 8), 1, what="two tiles")
    assert sorted(set(ref.tx.tolist())) == [3, 4] and set(ref.ty.tolist()) == {3}


# ---- 3: the adjoint identity on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,sk", [(64, (16, 4)), (65, (24, 12)), (64, (32, 16))], ids=str)
def test_adjoint_identity(ctx, N, sk):
    lam, n = LAMS[N], 500
    rng = np.random.default_rng(13)
    u, v = rng.uniform(-0.52 * lam, 0.52 * lam, n), rng.uniform(-0.52 * lam, 0.52 * lam, n)
    w = rng.uniform(-1500, 1500, n)
    w[5] = np.nan
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    ws = ctx.wstack(THETA, lam, tuple(to_dev(x) for x in (u, v, w)), fn(sk, 4))
    assert 1 < ws.dropped < n // 4
    lhs = np.sum(model * host(ws.image(to_dev(vis))))
    rhs = np.real(np.vdot(vis, host(ws.predict(to_dev(model))))) / (N * N)
    ws.close()
    print(f"N={N} {sk}: {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs))


# ---- 4: an imager -----------------------------------------------------------------------------------------------------------------------
def imager_against_the_calls(ctx, N, sk, M, span=0.4):
    import torch
    c = case(N, sk, M, n=600, span=span, seed=17)
    lam, f = c["lam"], fn(sk, M)
    im = ctx.imager(THETA, lam, dev3(c), f)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    r_img, r_psf, r_pmax = (host(x) if hasattr(x, "cpu") else x
                            for x in ctx.do_imaging(THETA, lam, dev3(c), None, None, None, None, dvis, f))
    r_pred = host(ctx.predict(THETA, lam, dev3(c), dmodel, f))
    r_img2 = host(ctx.do_imaging(THETA, lam, dev3(c), None, None, None, None, to_dev(c["vis"] - r_pred), f)[0])
    u1, v1, w1, vis1 = R.mirror_uvw(c["u"], c["v"], c["w"], c["vis"])
    wt = np.abs(R.doweight(N, u1 / np.float64(lam), v1 / np.float64(lam), np.ones(len(u1), dtype=np.complex128)))
    amp = lambda x: 2 * image_tol(N, sk[1], 2 * (wt * np.abs(x)).sum() / N ** 2 / r_pmax)  # noqa: E731
    pt = predict_tol(N, sk[1], c["model"])
    print(f"imager N={N} {sk} M={M}")
    within(host(im.psf), r_psf, amp(np.ones(len(wt))), "psf")
    assert abs(im.pmax - r_pmax) <= EPS * 2 * wt.sum() / N ** 2
    within(host(im.predict(dmodel)), r_pred, pt, "predict")
    for middle in (0, 1):
        ctx.set_option("wstack_middle", middle)
        try:
            within(host(im.cycle(dvis)), r_img, amp(c["vis"]), f"cycle (middle {middle})")
            res = torch.full_like(dvis, 7.0)
            within(host(im.cycle(dvis, dmodel, vis_res=res)), r_img2, amp(c["vis"] - r_pred), f"cycle(model) (middle {middle})")
            within(host(res), c["vis"] - r_pred, pt, f"vis_res (middle {middle})")
            buf = dvis.clone()
            within(host(im.cycle(buf, dmodel, vis_res=buf)), r_img2, amp(c["vis"] - r_pred), f"cycle in place (middle {middle})")
            within(host(buf), c["vis"] - r_pred, pt, f"vis_res in place (middle {middle})")
        finally:
            ctx.set_option("wstack_middle", 0)
    # and against the restatement
    n_img, n_psf, n_pmax = c["imaging"]
    within(host(im.cycle(dvis)), n_img, amp(c["vis"]), "cycle vs numpy")
    within(host(im.psf), n_psf, amp(np.ones(len(wt))), "psf vs numpy")
    assert ctx.get_option("errors") == 0
    im.close()


@pytest.mark.parametrize("N,sk,M", [(64, (24, 12), 4), (65, (16, 8), 1), (64, (32, 16), 4)], ids=str)
def test_an_imager_against_the_calls_it_replaces(ctx, N, sk, M):
    imager_against_the_calls(ctx, N, sk, M)


def test_an_imager_whose_two_streams_keep_different_visibilities(ctx):
    """0 <= x < N is not symmetric under the mirror for an odd N: with visibilities up to 0.52 lam the un-mirrored and the
    mirrored stream drop different ones, and every cycle takes the stream-order middle whatever the option says"""
    c = case(65, (16, 4), 4, n=600, span=0.52, seed=17)
    u1, v1, w1, _ = R.mirror_uvw(c["u"], c["v"], c["w"], c["vis"])
    plain, mirrored = c["ref"], I.Stack(THETA, c["lam"], u1, v1, w1, WSTEP, 4, 16, 4)
    assert plain.dropped > 0 and mirrored.dropped > 0 and not np.array_equal(plain.keep, mirrored.keep)
    imager_against_the_calls(ctx, 65, (16, 4), 4, span=0.52)


def test_an_imager_deconvolves_points_off_their_cell_centres(ctx):
    """Three points in the trusted region, each off its cell's centre, as exact dft_predict visibilities.  Peak cell: the
    model's largest component within two cells of a point lies in the point's own cell.  Flux: what the model carries at
    the point's true position - the least-squares amplitudes of the three true point responses in the model's own exact
    (dft_predict) visibilities - is the point's within 1 % at (24, 12).  (A sum of model cells around the point is no
    measure: the components of a point off its cell's centre alternate in sign and fall off slowly.)  The same figure is
    printed for the w-projection stack at support 15, for the record."""
    import gridhip
    N, lam, n = 64, 640, 600
    rng = np.random.default_rng(23)
    u, v = rng.uniform(-0.4 * lam, 0.4 * lam, n), rng.uniform(-0.4 * lam, 0.4 * lam, n)
    w = rng.uniform(-1500, 1500, n)
    px = np.array([[20, 40], [35, 27], [46, 22]])  # (y, x), inside cells 8 .. 56
    off = np.array([[0.1, -0.15], [-0.2, 0.1], [0.15, 0.2]])
    flux = np.array([1.0, 0.6, 0.8])
    pos = (px + off - N // 2) / N * THETA
    uvw = tuple(to_dev(x) for x in (u, v, w))
    dvis = ctx.dft_predict(uvw, to_dev(gridhip.components(pos[:, 1], pos[:, 0], flux))).clone()
    E = np.stack([host(ctx.dft_predict(uvw, to_dev(gridhip.components(pos[k:k + 1, 1], pos[k:k + 1, 0], [1.0]))))
                  for k in range(3)], axis=1)
    fns = {"idg (24, 12)": fn((24, 12), 4),
           "wstack S = 15": ("wstack", dict(wstep=WSTEP, planes=4, qpx=2, npixFF=32, npixKern=15))}
    for tag, f in fns.items():
        im = ctx.imager(THETA, lam, uvw, f)
        model, image, stats = im.deconvolve(dvis, 16, gain=0.1, niter=2000, border=8)
        m = host(model)
        yy, xx = np.nonzero(m)
        mc = gridhip.components((xx - N // 2) / N * THETA, (yy - N // 2) / N * THETA, m[yy, xx])
        got = np.linalg.lstsq(E, host(ctx.dft_predict(uvw, to_dev(mc))), rcond=None)[0].real
        peaks = [tuple(int(k) for k in np.unravel_index(np.argmax(np.abs(m[y - 2:y + 3, x - 2:x + 3])), (5, 5))) for y, x in px]
        worst = np.abs(got / flux - 1).max()
        print(f"{tag}: fluxes {got} of {flux} (worst {worst:.2e}), peak offsets {peaks}, {len(yy)} components, "
              f"residual {np.abs(host(image)).max():.2e}")
        if tag.startswith("idg"):
            assert all(p == (2, 2) for p in peaks)
            assert worst <= 0.01
        im.close()
    assert ctx.get_option("errors") == 0


def test_a_cycle_can_be_captured_into_a_graph(ctx):
    import torch
    c = case(65, (24, 12), 4, n=600, span=0.4, seed=17)
    N, sk = 65, (24, 12)
    im = ctx.imager(THETA, c["lam"], dev3(c), fn(sk, 4))
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    res, eager_res = torch.zeros_like(dvis), torch.zeros_like(dvis)
    eager = host(im.cycle(dvis, dmodel, vis_res=eager_res)).copy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        im.cycle(dvis, dmodel, out=img, vis_res=res)  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: no parallel branches
        im.cycle(dvis, dmodel, out=img, vis_res=res)
    torch.cuda.synchronize()
    img.fill_(7.0), res.fill_(7.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    r_pmax = c["imaging"][2]
    amp = 2 * (np.abs(c["vis"]) + np.abs(host(eager_res) - c["vis"])).sum() / N ** 2 / r_pmax  # (weights <= 1)
    within(host(img), eager, 2 * image_tol(N, sk[1], amp), "replayed cycle")
    assert np.array_equal(bits(host(res)), bits(host(eager_res))) and ctx.get_option("errors") == 0
    im.close()


# ---- 5: refusals at the C level -------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_handles_alone(ctx):
    import torch
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    c = case(64, (16, 4), 4)
    n = len(c["u"])
    du, dv, dw = dev3(c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    img = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
    psf = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
    out = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
    himg, hout = np.full((64, 64), 7.0), np.full(n, 7.0 + 0j)
    hu, hv, hw = (np.ascontiguousarray(c[k]) for k in "uvw")
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ctx.synchronize()
    bad = [(7, 4), (20, 8), (33, 16), (17, 8)] + [(16, K) for K in (2, 3, 5, 10)] + [(24, 14), (32, 18), (32, 0), (16, -4)]
    for S, K in bad:
        lead = (WSTEP, 4, 0, K, S, THETA, 640)
        ws = C.c_void_p(0x1234)
        assert lib.gridhip_wstack_create_dev(h, *lead, n, p(du), p(dv), p(dw), 1, C.byref(ws)) == _lib.EINVAL, (S, K)
        assert not ws.value
        pm = C.c_double(7.0)
        assert lib.gridhip_do_imaging_wstack_dev(h, *lead, n, p(du), p(dv), p(dw), 1, p(dvis), p(img), p(psf),
                                                 C.byref(pm)) == _lib.EINVAL
        assert lib.gridhip_do_imaging_wstack(h, *lead, n, hp(hu), hp(hv), hp(hw), 1, hp(c["vis"]), hp(himg), hp(himg),
                                             C.byref(pm)) == _lib.EINVAL
        assert lib.gridhip_predict_wstack_dev(h, *lead, p(dmodel), n, p(du), p(dv), p(dw), 1, None, p(out)) == _lib.EINVAL
        assert lib.gridhip_predict_wstack(h, *lead, hp(c["model"]), n, hp(hu), hp(hv), hp(hw), 1, None, hp(hout)) == _lib.EINVAL
        assert pm.value == 7.0
        for name in ("gridhip_imager_create_dev", "gridhip_imager_create_weighted_dev"):
            im = C.c_void_p(0x1234)
            tail = (2, 0.0, 0.0, None) if "weighted" in name else ()
            assert getattr(lib, name)(h, 4, WSTEP, 0, K, S, 4, None, THETA, 640, n, p(du), p(dv), p(dw), 1, *tail,
                                      C.byref(im)) == _lib.EINVAL, (name, S, K)
            assert not im.value
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and bool((psf == 7).all()) and bool((out == 7).all())
    assert (himg == 7).all() and (hout == 7).all()
    # the other kinds still refuse qpx = 0, and do_imaging / predict still refuse kind 4
    a = (4, WSTEP, 0, 8, 16, 4, None, THETA, 640, n, p(du), p(dv), p(dw), 1)
    pm = C.c_double(7.0)
    assert lib.gridhip_do_imaging_dev(h, *a, p(dvis), p(img), p(psf), C.byref(pm)) == _lib.EINVAL
    assert lib.gridhip_predict_dev(h, *a[:9], p(dmodel), *a[9:], None, p(out)) == _lib.EINVAL
    for kind in (3, 5, 2):
        im = C.c_void_p(0x1234)
        assert lib.gridhip_imager_create_dev(h, kind, *a[1:], C.byref(im)) == _lib.EINVAL and not im.value
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and bool((out == 7).all()) and pm.value == 7.0


# ---- 6: pre-filled scratch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x01], ids=["fillFF", "fill01"])
def test_on_pre_filled_scratch(fill):
    """a context of its own whose every block is filled with `fill` before it is used: image-domain layers read nothing
    they have not written (the tile-ordered arrays, the work items, the layer block, the grids)"""
    import gridhip
    own = gridhip.Context(0)
    try:
        own.set_option("scratch_fill", fill)  # before any other call
        before = own.get_option("scratch_filled")
        c = case(*PARITY[0])
        handle_parity(own, c)
        calls_parity(own, c)
        imager_against_the_calls(own, 64, (24, 12), 4)
        assert own.get_option("scratch_filled") > before and own.get_option("errors") == 0
    finally:
        own.close()
