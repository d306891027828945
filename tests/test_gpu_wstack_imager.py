"""The imager of the w-stacking kind on the GPU (gridhip_imager_create[_weighted]_dev with kind 4; Context.imager with
("wstack", kernops)) against the two calls it replaces, gridhip_do_imaging_wstack_dev and gridhip_predict_wstack_dev,
and against the numpy restatement tests/wstack_imager_ref.py.  Shapes and tolerance are tests/test_gpu_wstack.py's: 2000
visibilities, N = 64, 65 and 48, 1e-10 of the reference's largest magnitude (the gridder adds with fp64 atomics, so no
image is bit-reproducible; vis_res and the predictions of dropped visibilities are exact)."""
import ctypes as C

import numpy as np
import pytest

import wstack_imager_ref as WI
import wstack_ref as W
from test_gpu_wstack import NPIXFF, NVIS, SHAPES, TOL, WSTEP, case, host, opts, rel, to_dev

pytestmark = pytest.mark.gpu


def dev3(c, w=None):
    return to_dev(c["u"]), to_dev(c["v"]), to_dev(c["w"] if w is None else w)


def imgfn(c):
    return ("wstack", c["opts"])


def make(ctx, c, w=None, **kw):
    return ctx.imager(c["theta"], c["lam"], dev3(c, w), imgfn(c), **kw)


def do_imaging(ctx, c, vis, w=None):
    """the device form of the call the imager replaces -> (image, psf, pmax), numpy"""
    img, psf, pmax = ctx.do_imaging(c["theta"], c["lam"], dev3(c, w), None, None, None, None, to_dev(vis), imgfn(c))
    return host(img), host(psf), pmax


def predict(ctx, c, model, w=None):
    return host(ctx.predict(c["theta"], c["lam"], dev3(c, w), to_dev(model), imgfn(c)))


def bits(z):
    """the 64-bit patterns of a float64 or complex128 array, one row per element"""
    z = np.ascontiguousarray(z)
    return z.view(np.uint64).reshape(z.shape + (-1,))


_refs = {}


def restatement(c, key, M, S, Q):
    """the numpy imager of a case and its two cycles, computed once"""
    if key not in _refs:
        ref = WI.StackImager(c["theta"], c["lam"], c["u"], c["v"], c["w"], WSTEP, M, Q, NPIXFF, S)
        _refs[key] = (ref, ref.cycle(c["vis"])[0], ref.cycle(c["vis"], c["model"])[0])
    return _refs[key]


# ---- 1: against the calls it replaces, and against the restatement -------------------------------------------------------------
def against_the_calls(ctx, N, msq, L, n=NVIS):
    import torch
    c = case(N, msq, L, n=n)
    assert (c["v"] < 0).any() and (c["v"] >= 0).any() and (c["u"] < 0).any()
    im = make(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    r_img, r_psf, r_pmax = do_imaging(ctx, c, c["vis"])
    r_pred = predict(ctx, c, c["model"])
    r_img2 = do_imaging(ctx, c, c["vis"] - r_pred)[0]
    e = {"psf": rel(host(im.psf), r_psf), "pmax": abs(im.pmax - r_pmax) / r_pmax}
    e["cycle(None)"] = rel(host(im.cycle(dvis)), r_img)
    res = torch.full_like(dvis, 7.0)
    e["cycle(model)"] = rel(host(im.cycle(dvis, dmodel, vis_res=res)), r_img2)
    e["vis_res"] = rel(host(res), c["vis"] - r_pred)
    buf = dvis.clone()
    e["cycle, in place"] = rel(host(im.cycle(buf, dmodel, vis_res=buf)), r_img2)
    e["vis_res, in place"] = rel(host(buf), c["vis"] - r_pred)
    e["predict"] = rel(host(im.predict(dmodel)), r_pred)
    e["residual"] = rel(host(im.predict(dmodel, vis_sub=dvis)), c["vis"] - r_pred)
    buf = dvis.clone()
    assert im.predict(dmodel, vis_sub=buf, out=buf) is buf
    e["residual, in place"] = rel(host(buf), c["vis"] - r_pred)
    # the cycle again: the stack's grid is clear again
    e["cycle twice"] = rel(host(im.cycle(dvis, dmodel)), r_img2)
    e["cycle(None) twice"] = rel(host(im.cycle(dvis)), r_img)
    # the restatement
    ref, n_img, n_img2 = restatement(c, (N, msq, L, n), *msq)
    e["psf vs numpy"], e["pmax vs numpy"] = rel(host(im.psf), ref.psf), abs(im.pmax - ref.pmax) / ref.pmax
    e["cycle(None) vs numpy"] = rel(host(im.cycle(dvis)), n_img)
    e["cycle(model) vs numpy"] = rel(host(im.cycle(dvis, dmodel)), n_img2)
    e["predict vs numpy"] = rel(host(im.predict(dmodel)), c["pred"])
    print(f"N={N} {msq} L={L}:", {k: f"{x:.2e}" for k, x in e.items()})
    assert max(e.values()) < TOL, e
    assert ctx.get_option("errors") == 0
    im.close()


CALLS = [(64, (4, 7, 4), 9), (65, (5, 9, 2), 16), (48, (3, 7, 1), 9), (65, (1, 9, 2), 1)]


@pytest.mark.parametrize("N,msq,L", CALLS)
def test_against_the_calls_it_replaces(ctx, N, msq, L):
    against_the_calls(ctx, N, msq, L)


# ---- 2: the two partitions differ ----------------------------------------------------------------------------------------------------
def partition_stream(signs):
    """w >= 0 in the planes 0 .. 16 with M = 4: the un-mirrored stream has 5 layers, all occupied, the last one holding plane
    16 alone.  signs "both": v < 0 exactly where the plane is >= 8, so the mirrored stream has the planes -16 .. -8 and
    0 .. 7: 6 layers from pmin = -16, layer 2 holding plane -8 alone (a partial layer) and layer 3 (planes -4 .. -1) empty
    in the middle.  "negative": every plane is negated, 5 layers from pmin = -16.  "not negative": nothing is mirrored."""
    N = 65
    theta, lam = SHAPES[N]
    rng = np.random.default_rng(51)
    n = 700
    p = rng.integers(0, 17, n)
    p[:3] = [0, 16, 8]
    w = p * float(WSTEP) + rng.uniform(0.0, 40.0, n)  # (rounds to p; never negative)
    w[0] = 0.0
    u = rng.uniform(-0.4 * lam, 0.4 * lam, n)
    a = rng.uniform(0.01 * lam, 0.4 * lam, n)
    if signs == "both":
        v = np.where(p >= 8, -a, a)
    elif signs == "negative":
        v = -a
    else:
        v = a.copy()
        v[5], v[6], v[7], v[8] = -0.0, 0.0, -0.0, 0.0  # (a zero of either sign is not mirrored)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    return dict(theta=theta, lam=lam, N=N, u=u, v=v, w=w, vis=vis, model=model, opts=opts(4, 7, 4))


@pytest.mark.parametrize("signs", ["both", "negative", "not negative"])
def test_the_two_partitions_differ(ctx, signs):
    c = partition_stream(signs)
    neg = c["v"] < 0
    plain, mirrored = W.layers(c["w"], WSTEP, 4), W.layers(np.where(neg, -c["w"], c["w"]), WSTEP, 4)
    occ = lambda lay: sorted(set(lay["layer"].tolist()))  # noqa: E731
    assert (plain["L"], plain["pmin"], occ(plain)) == (5, 0, [0, 1, 2, 3, 4]) and np.sum(plain["layer"] == 4) >= 1
    if signs == "both":
        assert (mirrored["L"], mirrored["pmin"]) == (6, -16) and occ(mirrored) == [0, 1, 2, 4, 5]
        assert set(mirrored["r"][mirrored["layer"] == 2].tolist()) == {0}  # (plane -8 alone: a partial layer)
    elif signs == "negative":
        assert (mirrored["L"], mirrored["pmin"]) == (5, -16) and np.sum(mirrored["layer"] == 0) >= 1
    else:
        assert not neg.any() and np.signbit(c["v"][5]) and mirrored["L"] == 5
    # the device's own stacks on the two streams have those layers
    for lay, w in ((plain, c["w"]), (mirrored, np.where(neg, -c["w"], c["w"]))):
        s = np.where(neg, -1.0, 1.0)
        ws = ctx.wstack(c["theta"], c["lam"], (to_dev(c["u"] * s if lay is mirrored else c["u"]),
                                               to_dev(c["v"] * s if lay is mirrored else c["v"]), to_dev(w)), c["opts"])
        assert (ws.layers, ws.occupied, ws.pmin) == (lay["L"], len(occ(lay)), lay["pmin"])
        ws.close()
    im = make(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    r_img, r_psf, r_pmax = do_imaging(ctx, c, c["vis"])
    r_pred = predict(ctx, c, c["model"])
    r_img2 = do_imaging(ctx, c, c["vis"] - r_pred)[0]
    e = {"psf": rel(host(im.psf), r_psf), "pmax": abs(im.pmax - r_pmax) / r_pmax,
         "cycle(None)": rel(host(im.cycle(dvis)), r_img), "predict": rel(host(im.predict(dmodel)), r_pred)}
    res = to_dev(np.zeros(len(c["vis"]), dtype=np.complex128))
    e["cycle(model)"] = rel(host(im.cycle(dvis, dmodel, vis_res=res)), r_img2)
    e["vis_res"] = rel(host(res), c["vis"] - r_pred)
    ctx.set_option("wstack_middle", 1)
    try:
        e["cycle(model), other middle"] = rel(host(im.cycle(dvis, dmodel)), r_img2)
    finally:
        ctx.set_option("wstack_middle", 0)
    ref = WI.StackImager(c["theta"], c["lam"], c["u"], c["v"], c["w"], WSTEP, 4, 4, NPIXFF, 7)
    e["cycle(model) vs numpy"] = rel(host(im.cycle(dvis, dmodel)), ref.cycle(c["vis"], c["model"])[0])
    print(signs, {k: f"{x:.2e}" for k, x in e.items()})
    assert max(e.values()) < TOL, e
    assert ctx.get_option("errors") == 0
    im.close()


# ---- 3: dropped samples, the grid's edge ------------------------------------------------------------------------------------------------
BAD = [3, 777, 1200, NVIS - 1]


def dropped_samples(ctx):
    import torch
    c = case(64, (5, 9, 2), 9)
    w = c["w"].copy()
    w[BAD] = [np.nan, np.inf, -np.inf, np.nan]
    vis = c["vis"].copy()
    vis[777] = np.nan + 1j * np.nan
    keep = np.ones(NVIS, dtype=bool)
    keep[BAD] = False
    dvis, dmodel = to_dev(vis), to_dev(c["model"])
    e = {}
    # natural weights, so that the stream without the samples has the same weights: the images are equal
    im = make(ctx, c, w, weighting="natural")
    assert ctx.last_dropped() == len(BAD)
    short = ctx.imager(c["theta"], c["lam"], tuple(to_dev(x[keep]) for x in (c["u"], c["v"], c["w"])), imgfn(c),
                       weighting="natural")
    e["psf without them"] = rel(host(im.psf), host(short.psf))
    for m in (None, dmodel):
        for middle in (0, 1):
            ctx.set_option("wstack_middle", middle)
            try:
                want = host(short.cycle(to_dev(vis[keep]), m))
                res = torch.full_like(dvis, 7.0)
                got = host(im.cycle(dvis, m, vis_res=res))
                assert ctx.last_dropped() == len(BAD)
                buf = dvis.clone()
                got2 = host(im.cycle(buf, m, vis_res=buf))
            finally:
                ctx.set_option("wstack_middle", 0)
            tag = f"{'model' if m is not None else 'no model'}, middle {middle}"
            e[f"image ({tag})"], e[f"image in place ({tag})"] = rel(got, want), rel(got2, want)
            assert np.isfinite(got).all()
            # vis_res[k] has the bits of vis[k], the NaN's among them
            assert np.array_equal(bits(host(res))[BAD], bits(vis)[BAD]), tag
            assert np.array_equal(bits(host(buf))[BAD], bits(vis)[BAD]), tag
            assert np.array_equal(host(buf)[keep], host(res)[keep]), tag
    pred = host(im.predict(dmodel))
    assert np.all(bits(pred)[BAD] == 0)  # exactly +0
    out = host(im.predict(dmodel, vis_sub=dvis))
    assert np.array_equal(bits(out)[BAD], bits(vis)[BAD])
    e["predict"] = rel(pred[keep], host(short.predict(dmodel)))
    im.close(), short.close()
    # the default weights count the dropped samples' cells, as the call it replaces does
    im = make(ctx, c, w)
    r_img, r_psf, r_pmax = do_imaging(ctx, c, vis, w)
    assert ctx.last_dropped() == len(BAD)
    e["psf vs do_imaging"], e["pmax vs do_imaging"] = rel(host(im.psf), r_psf), abs(im.pmax - r_pmax) / r_pmax
    e["image vs do_imaging"] = rel(host(im.cycle(dvis)), r_img)
    print({k: f"{x:.2e}" for k, x in e.items()})
    assert max(e.values()) < TOL, e
    assert ctx.get_option("errors") == 0
    im.close()


def test_dropped_samples(ctx):
    dropped_samples(ctx)


def test_visibilities_at_the_grid_edge(ctx):
    """u, v up to +-0.5 lam and a little beyond (tests/test_gpu_wstack.py's stream): footprints cut by the grid's border"""
    for N, msq in [(64, (4, 7, 4)), (65, (5, 9, 2))]:
        c = case(N, msq, 9, seed=31, span=0.56)
        im = make(ctx, c)
        dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
        r_img, r_psf, r_pmax = do_imaging(ctx, c, c["vis"])
        r_pred = predict(ctx, c, c["model"])
        e = [rel(host(im.psf), r_psf), rel(host(im.cycle(dvis)), r_img), rel(host(im.predict(dmodel)), r_pred),
             rel(host(im.cycle(dvis, dmodel)), do_imaging(ctx, c, c["vis"] - r_pred)[0]),
             rel(host(im.predict(dmodel)), c["pred"])]
        print(N, e)
        assert max(e) < TOL and np.any(host(im.predict(dmodel)) == 0) and ctx.get_option("errors") == 0
        im.close()


# ---- 4: weighted creation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["natural", "briggs"])
def test_weighted_creation_is_weights_composed_with_the_mirrored_stack(ctx, mode):
    c = case(65, (4, 7, 4), 9)
    rng = np.random.default_rng(61)
    s = rng.uniform(0.5, 2.0, NVIS)
    flagged = rng.random(NVIS) < 0.1
    s[flagged] = 0.0
    k0 = int(np.flatnonzero(flagged)[0])
    vis = c["vis"].copy()
    vis[k0] = np.nan + 1j * np.nan  # a zero weight under a NaN
    # by hand: mirror, Context.weights of the mirrored stream, a stack on the mirrored stream
    uvw1, vis1 = ctx.mirror_uvw((c["u"], c["v"], c["w"]), vis)
    wt, st = ctx.weights(c["theta"], c["lam"], uvw1, mode, 0.3, 0.0, s)
    assert wt[k0] == 0 and (wt[~flagged] > 0).all()
    ws = ctx.wstack(c["theta"], c["lam"], tuple(to_dev(x) for x in uvw1), c["opts"])
    with np.errstate(invalid="ignore"):
        x = np.where(wt > 0, wt * vis1, 0.0)
    psf = 2.0 * host(ws.image(to_dev(wt.astype(np.complex128))))
    pmax = psf.max()
    img = 2.0 * host(ws.image(to_dev(x))) / pmax
    ws.close()
    im = make(ctx, c, weighting=mode, robust=0.3, weights=to_dev(s))
    psf_before = host(im.psf).copy()
    got = host(im.cycle(to_dev(vis)))
    e = {"image": rel(got, img), "psf": rel(host(im.psf), psf / pmax), "pmax": abs(im.pmax - pmax) / pmax,
         "stats": np.abs(host(im.weight_stats()) - st).max() / np.abs(st).max()}
    # the flagged samples: nothing of them in any image - the imager of the stream without them gives the same
    keep = ~flagged
    short = ctx.imager(c["theta"], c["lam"], tuple(to_dev(c[k][keep]) for k in "uvw"), imgfn(c), weighting=mode, robust=0.3,
                       weights=to_dev(s[keep]))
    e["image without them"] = rel(got, host(short.cycle(to_dev(vis[keep]))))
    e["psf without them"] = rel(host(im.psf), host(short.psf))
    print(mode, {k: f"{v:.2e}" for k, v in e.items()})
    assert np.isfinite(got).all() and np.isfinite(host(im.psf)).all()
    # the NaN under the zero weight has touched no bit of the PSF the imager keeps
    im._psf = None
    assert np.array_equal(bits(host(im.psf)), bits(psf_before))
    assert max(e.values()) < TOL, e
    assert ctx.get_option("errors") == 0
    im.close(), short.close()


# ---- 5: the two middle paths -----------------------------------------------------------------------------------------------------------
def test_the_two_middle_paths_agree(ctx):
    import torch
    c = case(65, (5, 9, 2), 16)
    w = c["w"].copy()
    w[[11, 500]] = [np.inf, np.nan]
    dmodel = to_dev(c["model"])
    for stream_w, tag in ((None, "all finite"), (w, "dropped")):
        im = make(ctx, c, stream_w)
        dvis = to_dev(c["vis"])
        want = host(im.predict(dmodel, vis_sub=dvis))
        for m in (dmodel, None):
            out = {}
            for middle in (0, 1):
                ctx.set_option("wstack_middle", middle)
                try:
                    assert ctx.get_option("wstack_middle") == middle
                    res = torch.full_like(dvis, 7.0)
                    img = host(im.cycle(dvis, m, vis_res=res))
                    buf = dvis.clone()
                    img2 = host(im.cycle(buf, m, vis_res=buf))
                finally:
                    ctx.set_option("wstack_middle", 0)
                out[middle] = (img, host(res), img2, host(buf))
            a, b = out[0], out[1]
            assert np.array_equal(bits(a[1]), bits(b[1])), tag      # vis_res bit for bit
            assert np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(bits(a[1]), bits(a[3])), tag  # and in place
            assert np.array_equal(bits(a[1]), bits(want if m is not None else c["vis"])), tag  # = Imager.predict's residual
            e = [rel(a[0], b[0]), rel(a[2], b[0]), rel(b[2], b[0])]
            print(tag, "model" if m is not None else "no model", e)
            assert max(e) < TOL and np.abs(b[0]).max() > 0
        assert ctx.get_option("errors") == 0
        im.close()


# ---- 6: the imager's surface -----------------------------------------------------------------------------------------------------------
def mfs_cycle_against_cycles(ctx):
    import torch
    T = 2
    c = case(64, (4, 7, 4), 9)
    im = make(ctx, c)
    x = to_dev(np.random.default_rng(5).choice(np.linspace(-0.2, 0.2, 8), NVIS))
    dvis = to_dev(c["vis"])
    im.set_spectral(x, T)
    psfs = host(im.spectral_psfs())
    e = {"P_0 vs psf": np.abs(psfs[0] - host(im.psf)).max()}
    for s in range(2 * T - 1):
        e[f"P_{s}"] = np.abs(psfs[s] - host(im.cycle((x ** s).to(torch.complex128)))).max()  # (in units of pmax)
    models = to_dev(np.random.default_rng(3).normal(size=(T, 64, 64)))
    r = dvis.clone()
    for q in range(T):
        r = r - x ** q * im.predict(models[q])
    want = torch.stack([im.cycle((x ** t * r).contiguous()) for t in range(T)])
    res = torch.full_like(dvis, 7.0)
    e["images"] = rel(host(im.mfs_cycle(dvis, models, vis_res=res)), host(want))
    e["vis_res"] = rel(host(res), host(r))
    want0 = torch.stack([im.cycle((x ** t * dvis).contiguous()) for t in range(T)])
    e["images, no models"] = rel(host(im.mfs_cycle(dvis)), host(want0))
    print({k: f"{v:.2e}" for k, v in e.items()})
    assert np.abs(psfs[1]).max() > 0 and np.abs(host(want)[1]).max() > 0
    assert max(e.values()) < TOL, e
    assert ctx.get_option("errors") == 0
    im.close()


def test_mfs_cycle_against_cycle_calls(ctx):
    mfs_cycle_against_cycles(ctx)


def test_deconvolve_is_the_loop_of_cycle_and_clean(ctx):
    c = case(64, (4, 7, 4), 9)
    im = make(ctx, c)
    sky = np.zeros((64, 64))
    sky[20, 40], sky[35, 30], sky[44, 22] = 1.0, 0.6, -0.4
    dvis = im.predict(to_dev(sky)).clone()
    kw = dict(gain=0.2, niter=30)
    model, image, stats = im.deconvolve(dvis, 2, **kw)
    m2 = to_dev(np.zeros((64, 64)))
    rows = []
    for _ in range(2):
        res = im.cycle(dvis, m2)
        m2, res, st = ctx.clean(res, im.psf, model=m2, **kw)
        rows.append(host(st))
    closing = host(im.cycle(dvis, m2))
    e = [rel(host(model), host(m2)), rel(host(image), closing), np.abs(host(stats)[:, [0, 2]] - np.array(rows)[:, [0, 2]]).max()]
    print(e, host(stats))
    assert np.abs(host(m2)).max() > 0 and host(stats)[0, 0] == 30
    assert e[0] < TOL and e[1] < TOL and e[2] == 0
    assert ctx.get_option("errors") == 0
    im.close()


def test_selfcal_is_predict_gaincal_apply(ctx):
    c = case(64, (4, 7, 4), 9)
    im = make(ctx, c)
    rng = np.random.default_rng(71)
    nant = 8
    a1 = rng.integers(0, nant - 1, NVIS)
    a2 = a1 + 1 + rng.integers(0, nant - 1 - a1)
    gt = (1.0 + 0.1 * rng.normal(size=(1, nant))) * np.exp(1j * 0.3 * rng.normal(size=(1, nant)))
    sky = np.zeros((64, 64))
    sky[30, 34], sky[22, 41] = 1.0, 0.5
    dm, d1, d2 = to_dev(sky), to_dev(a1), to_dev(a2)
    vis = ctx.apply_gains(to_dev(gt), im.predict(dm), d1, d2, inverse=False)[0].clone()
    kw = dict(niter=100, tol=0.0)  # (a fixed count, far past convergence)
    g0, st0 = ctx.gaincal(vis, im.predict(dm), d1, d2, nant, **kw)
    v0, w0 = ctx.apply_gains(g0, vis, d1, d2)
    g1, v1, w1, st1 = im.selfcal(dm, vis, d1, d2, nant, **kw)
    G0, G1, V0, V1, W0, W1, S0, S1 = (host(t) for t in (g0, g1, v0, v1, w0, w1, st0, st1))
    scale = np.abs(G0).max()
    print(f"gains {np.abs(G1 - G0).max() / scale:.2e} vis {np.abs(V1 - V0).max() / np.abs(V0).max():.2e} stats {S1}")
    assert np.abs(G1 - G0).max() <= TOL * scale and np.abs(V1 - V0).max() <= 1e-9 * np.abs(V0).max()
    assert np.allclose(W1, W0, rtol=1e-9, atol=0) and S1[0] == 100 and S1[0] == S0[0]
    assert ctx.get_option("errors") == 0
    im.close()


# ---- 7: capture and allocation -----------------------------------------------------------------------------------------------------------
def test_a_cycle_can_be_captured_into_a_graph(ctx):
    import torch
    c = case(65, (4, 7, 4), 9)
    im = make(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = torch.zeros((65, 65), dtype=torch.float64, device="cuda:0")
    res = torch.zeros_like(dvis)
    eager_res = torch.zeros_like(dvis)
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
    e = rel(host(img), eager)
    print(e)
    assert e < TOL and np.array_equal(bits(host(res)), bits(host(eager_res))) and ctx.get_option("errors") == 0
    im.close()


def test_a_second_cycle_and_predict_allocate_nothing(ctx):
    import torch
    c = case(64, (5, 9, 2), 16)
    im = make(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = torch.zeros((64, 64), dtype=torch.float64, device="cuda:0")
    out, res = torch.zeros_like(dvis), torch.zeros_like(dvis)
    for middle in (1, 0):
        ctx.set_option("wstack_middle", middle)
        try:
            im.cycle(dvis, dmodel, out=img, vis_res=res), im.predict(dmodel, vis_sub=dvis, out=out)
            torch.cuda.synchronize()
            free = torch.cuda.mem_get_info()[0]
            im.cycle(dvis, dmodel, out=img, vis_res=res), im.cycle(dvis, out=img), im.predict(dmodel, out=out)
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free
        finally:
            ctx.set_option("wstack_middle", 0)
    assert rel(host(out), c["pred"]) < TOL and ctx.get_option("errors") == 0
    im.close()


# ---- 8: isolation and limits ---------------------------------------------------------------------------------------------------------------
def test_other_stacks_between_two_cycles_change_nothing(ctx):
    c, other = case(64, (4, 7, 4), 9), case(48, (3, 7, 1), 9)
    im = make(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    first = host(im.cycle(dvis, dmodel))
    do_imaging(ctx, other, other["vis"])
    second_im = make(ctx, other)
    second_im.cycle(to_dev(other["vis"]), to_dev(other["model"]))
    again = host(im.cycle(dvis, dmodel))
    second_im.close()
    third = host(im.cycle(dvis, dmodel))
    assert rel(again, first) < TOL and rel(third, first) < TOL and ctx.get_option("errors") == 0
    im.close()


def test_an_empty_stream_and_a_stream_without_a_finite_w(ctx):
    import torch
    c = case(48, (3, 7, 1), 9)
    e = torch.zeros(0, dtype=torch.float64, device="cuda:0")
    im = ctx.imager(c["theta"], c["lam"], (e, e, e), imgfn(c))
    img = torch.full((48, 48), 7.0, dtype=torch.float64, device="cuda:0")
    im.cycle(torch.zeros(0, dtype=torch.complex128, device="cuda:0"), out=img)
    assert not bool(img.any()) and not bool(im.psf.any())
    assert im.predict(to_dev(c["model"])).shape == (0,)
    im.close()
    # no finite w: whatever do_imaging's division by pmax = 0 leaves, NaN for NaN
    n = 50
    w = np.full(n, np.nan)
    w[::2] = np.inf
    s = dict(c, u=c["u"][:n], v=c["v"][:n], w=w)
    r_img, r_psf, r_pmax = do_imaging(ctx, s, c["vis"][:n])
    im = make(ctx, s)
    assert ctx.last_dropped() == n
    got = host(im.cycle(to_dev(c["vis"][:n])))
    assert np.array_equal(got, r_img, equal_nan=True) and np.array_equal(host(im.psf), r_psf, equal_nan=True)
    assert im.pmax == r_pmax or (np.isnan(im.pmax) and np.isnan(r_pmax))
    assert np.all(bits(host(im.predict(to_dev(c["model"])))) == 0)
    res = to_dev(np.zeros(n, dtype=np.complex128))
    im.cycle(to_dev(c["vis"][:n]), to_dev(c["model"]), vis_res=res)
    assert np.array_equal(host(res), c["vis"][:n]) and ctx.get_option("errors") == 0
    im.close()


def test_refusals_leave_the_handle_null(ctx):
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    c = case(64, (4, 7, 4), 9)
    du, dv, dw = dev3(c)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(kind=4, wstep=WSTEP, Q=4, ff=NPIXFF, gh=7, gw=4, kv=None, theta=c["theta"], lam=c["lam"], n=NVIS, u=p(du),
                v=p(dv), w=p(dw), st=1)
    order = ("kind", "wstep", "Q", "ff", "gh", "gw", "kv", "theta", "lam", "n", "u", "v", "w", "st")
    ctx.synchronize()
    for bad in (dict(gw=0), dict(gw=-1), dict(wstep=0), dict(gh=17), dict(ff=5, gh=5), dict(Q=0), dict(w=None), dict(u=None),
                dict(kind=3), dict(kind=5)):
        a = [dict(good, **bad)[k] for k in order]
        im = C.c_void_p(0x1234)
        assert lib.gridhip_imager_create_dev(h, *a, C.byref(im)) == _lib.EINVAL, bad
        assert not im.value, bad
        im = C.c_void_p(0x1234)
        assert lib.gridhip_imager_create_weighted_dev(h, *a, 2, 0.0, 0.0, None, C.byref(im)) == _lib.EINVAL, bad
        assert not im.value, bad
    # do_imaging and predict keep refusing the kind: they have their _wstack forms
    a = [good[k] for k in order]
    import torch
    img = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
    out = torch.full((NVIS,), 7.0, dtype=torch.complex128, device="cuda:0")
    pm = C.c_double(7.0)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    assert lib.gridhip_do_imaging_dev(h, *a, p(dvis), p(img), p(img), C.byref(pm)) == _lib.EINVAL
    assert lib.gridhip_predict_dev(h, *a[:9], p(dmodel), *a[9:], None, p(out)) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and bool((out == 7).all()) and pm.value == 7.0


def test_too_many_layers_is_unsupported(ctx):
    import gridhip
    from gridhip import _lib
    theta, lam = SHAPES[48]
    rng = np.random.default_rng(41)
    n = 64
    u, v = rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)
    w = np.zeros(n)
    w[1] = 4096.0 * WSTEP  # planes 0 .. 4096 with M = 1: 4097 layers on the un-mirrored stream
    v[1] = abs(v[1])
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.imager(theta, lam, tuple(to_dev(x) for x in (u, v, w)), ("wstack", opts(1, 7, 2)))
    assert ei.value.code == _lib.EUNSUPPORTED
    # 4096 layers on the stream as given, 4097 on the mirrored one (planes -2048 .. 2048): the second stack refuses
    w[1], w[2] = 2048.0 * WSTEP, 2048.0 * WSTEP
    v[1], v[2] = -abs(v[1]) - 1.0, abs(v[2]) + 1.0
    w[3] = -2047.0 * WSTEP
    v[3] = abs(v[3]) + 1.0
    assert W.layers(w, WSTEP, 1)["L"] == 4096 and W.layers(np.where(v < 0, -w, w), WSTEP, 1)["L"] == 4097
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.imager(theta, lam, tuple(to_dev(x) for x in (u, v, w)), ("wstack", opts(1, 7, 2)))
    assert ei.value.code == _lib.EUNSUPPORTED
    assert ctx.get_option("errors") == 0


# ---- 9: pre-filled scratch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x01], ids=["fillFF", "fill01"])
def test_on_pre_filled_scratch(fill):
    """a context of its own whose every block is filled with `fill` before it is used: a kind-4 imager reads nothing it has
    not written (both stacks' layer blocks, the composed index, the borrowed tables and grids)"""
    import gridhip
    own = gridhip.Context(0)
    try:
        own.set_option("scratch_fill", fill)  # before any other call
        before = own.get_option("scratch_filled")
        against_the_calls(own, *CALLS[0])
        dropped_samples(own)
        mfs_cycle_against_cycles(own)
        assert own.get_option("scratch_filled") > before and own.get_option("errors") == 0
    finally:
        own.close()
