"""W-stacking on the GPU (gridhip_wstack*, gridhip_do_imaging_wstack*, gridhip_predict_wstack*; Context.wstack, and
("wstack", ...) in Context.do_imaging / Context.predict) against the numpy restatement tests/wstack_ref.py.
The tolerance is the project's own: 1e-10 of the reference's largest magnitude (the gridder adds with fp64 atomics, so
neither side is bit-reproducible).  Shapes: N = 64 (even), 65 (odd), 48 (no multiple of a 16-cell tile); 2000
visibilities; (M, S, qpx) with M = 1, even and odd M and qpx = 1; w ranges that give 1, 9 and 16 layers."""
import ctypes as C

import numpy as np
import pytest

import wstack_ref as W

pytestmark = pytest.mark.gpu

TOL = 1e-10
WSTEP, NPIXFF, NVIS = 100, 16, 2000
SHAPES = {64: (0.1, 640), 65: (0.1, 650), 48: (0.15, 320)}
MSQ = [(1, 9, 2), (4, 7, 4), (5, 9, 2), (3, 7, 1)]


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


def opts(M, S, Q):
    return dict(wstep=WSTEP, planes=M, qpx=Q, npixFF=NPIXFF, npixKern=S)


def make_w(rng, n, M, L, partial=False):
    """w whose planes span exactly L layers of M planes around 0: the lowest and the highest plane are both taken (the
    last layer holds its first plane alone when `partial`)"""
    span = (L - 1) * M if partial else L * M - 1
    pmin = -(span // 2)
    w = rng.uniform(pmin * WSTEP, (pmin + span) * WSTEP, n)
    w[0], w[1] = pmin * WSTEP, (pmin + span) * WSTEP
    return w


_cases = {}


def case(N, msq, L, seed=11, span=0.4, partial=False, n=NVIS):
    """a stream of n visibilities, a model, the restatement's plan and its outputs, computed once per (shape, kernel,
    layers, n)"""
    key = (N, msq, L, seed, span, partial, n)
    if key not in _cases:
        theta, lam = SHAPES[N]
        M, S, Q = msq
        rng = np.random.default_rng(seed)
        u, v = rng.uniform(-span * lam, span * lam, n), rng.uniform(-span * lam, span * lam, n)
        w = make_w(rng, n, M, L, partial)
        vis = rng.normal(size=n) + 1j * rng.normal(size=n)
        model = rng.normal(size=(N, N))
        ref = W.Stack(theta, lam, u, v, w, WSTEP, M, Q, NPIXFF, S)
        _cases[key] = dict(theta=theta, lam=lam, N=N, u=u, v=v, w=w, vis=vis, model=model, ref=ref, opts=opts(M, S, Q),
                           image=ref.image(vis), pred=ref.predict(model))
    return _cases[key]


def bind(ctx, c):
    return ctx.wstack(c["theta"], c["lam"], tuple(to_dev(c[k]) for k in "uvw"), c["opts"])


# ---- 1: the handle's two passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 9, 16])
@pytest.mark.parametrize("msq", MSQ, ids=lambda x: "M%d-S%d-Q%d" % x)
@pytest.mark.parametrize("N", [64, 65, 48])
def test_image_and_predict(ctx, N, msq, L):
    import torch
    c = case(N, msq, L)
    ws = bind(ctx, c)
    assert ws.layers == c["ref"].lay["L"] == L and ws.occupied == len(c["ref"].occupied) and ws.dropped == 0
    assert ws.pmin == c["ref"].lay["pmin"]
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = host(ws.image(dvis))
    pred = host(ws.predict(dmodel))
    e_img, e_pred = rel(img, c["image"]), rel(pred, c["pred"])
    res = host(ws.predict(dmodel, vis_sub=dvis))
    inplace = dvis.clone()
    assert ws.predict(dmodel, vis_sub=inplace, out=inplace) is inplace
    torch.cuda.synchronize()
    e_res, e_inp = rel(res, c["vis"] - c["pred"]), rel(host(inplace), c["vis"] - c["pred"])
    # a second image pass finds the grid clear again
    e_img2 = rel(host(ws.image(dvis)), c["image"])
    print(f"N={N} {msq} L={L}: image {e_img:.2e} {e_img2:.2e} predict {e_pred:.2e} residual {e_res:.2e} in place {e_inp:.2e}")
    assert max(e_img, e_img2, e_pred, e_res, e_inp) < TOL and ctx.get_option("errors") == 0
    ws.close()


# ---- 2: do_imaging and predict, host and device forms -------------------------------------------------------------------------
@pytest.mark.parametrize("N,msq,L", [(64, (4, 7, 4), 9), (65, (5, 9, 2), 16), (48, (3, 7, 1), 9), (65, (1, 9, 2), 1)])
def test_do_imaging_and_predict_host_and_device(ctx, N, msq, L):
    c = case(N, msq, L)
    theta, lam, o = c["theta"], c["lam"], c["opts"]
    M, S, Q = msq
    r_img, r_psf, r_pmax = W.do_imaging(theta, lam, c["u"], c["v"], c["w"], c["vis"], WSTEP, M, Q, NPIXFF, S)
    uvw = np.stack([c["u"], c["v"], c["w"]], axis=1)  # the (n, 3) matrix: stride 3
    img, psf, pmax = ctx.do_imaging(theta, lam, uvw, None, None, None, None, c["vis"], ("wstack", o))
    dimg, dpsf, dpmax = ctx.do_imaging(theta, lam, tuple(to_dev(c[k]) for k in "uvw"), None, None, None, None,
                                       to_dev(c["vis"]), ("wstack", o))
    errs = [rel(img, r_img), rel(psf, r_psf), abs(pmax - r_pmax) / r_pmax, rel(host(dimg), img), rel(host(dpsf), psf),
            abs(dpmax - pmax) / pmax]
    pred = ctx.predict(theta, lam, uvw, c["model"], ("wstack", o))
    dpred = ctx.predict(theta, lam, to_dev(uvw), to_dev(c["model"]), ("wstack", o))
    sub = c["vis"].copy()
    assert ctx.predict(theta, lam, (c["u"], c["v"], c["w"]), c["model"], ("wstack", o), vis_sub=sub, out=sub) is sub
    errs += [rel(pred, c["pred"]), rel(host(dpred), pred), rel(sub, c["vis"] - c["pred"])]
    print(f"N={N} {msq} L={L}:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL and isinstance(img, np.ndarray) and dimg.is_cuda


# ---- 3: layers that are empty or partial, dropped visibilities, the grid's edge -------------------------------------------------
def test_empty_middle_layer_and_partial_last_layer(ctx):
    N, (M, S, Q) = 65, (4, 7, 4)
    theta, lam = SHAPES[N]
    rng = np.random.default_rng(21)
    n = 600
    u, v = rng.uniform(-0.4 * lam, 0.4 * lam, n), rng.uniform(-0.4 * lam, 0.4 * lam, n)
    # planes -6 .. -3 (layer 0), nothing in layers 1 and 2, planes 6 .. 9 (layer 3), plane 10 alone in layer 4
    w = np.concatenate([rng.uniform(-640, -260, 300), rng.uniform(560, 940, 299), [1000.0]])
    w[0], w[300] = -600.0, 600.0
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    ref = W.Stack(theta, lam, u, v, w, WSTEP, M, Q, NPIXFF, S)
    assert ref.lay["L"] == 5 and ref.occupied == [0, 3, 4] and np.sum(ref.lay["layer"] == 4) == 1
    ws = ctx.wstack(theta, lam, (to_dev(u), to_dev(v), to_dev(w)), opts(M, S, Q))
    assert (ws.layers, ws.occupied, ws.pmin, ws.dropped) == (5, 3, -6, 0)
    e = [rel(host(ws.image(to_dev(vis))), ref.image(vis)), rel(host(ws.predict(to_dev(model))), ref.predict(model))]
    print(e)
    assert max(e) < TOL
    ws.close()


def test_a_non_finite_w_is_dropped_and_predicts_zero(ctx):
    c = case(64, (5, 9, 2), 9)
    w = c["w"].copy()
    bad = [3, 777, NVIS - 1]
    w[3], w[777], w[NVIS - 1] = np.nan, np.inf, -np.inf
    ref = W.Stack(c["theta"], c["lam"], c["u"], c["v"], w, WSTEP, 5, 2, NPIXFF, 9)
    ws = ctx.wstack(c["theta"], c["lam"], (to_dev(c["u"]), to_dev(c["v"]), to_dev(w)), c["opts"])
    assert ws.dropped == 3 and ws.layers == ref.lay["L"]
    dvis = to_dev(c["vis"])
    img = host(ws.image(dvis))
    assert ctx.last_dropped() == 3
    pred = host(ws.predict(to_dev(c["model"])))
    res = host(ws.predict(to_dev(c["model"]), vis_sub=dvis))
    assert ctx.last_dropped() == 3
    assert np.all(pred[bad] == 0) and np.array_equal(res[bad], c["vis"][bad])
    e = [rel(img, ref.image(c["vis"])), rel(pred, ref.predict(c["model"])), rel(res, ref.predict(c["model"], c["vis"]))]
    print(e)
    assert max(e) < TOL
    ws.close()
    # the one-call forms count them too
    out = ctx.predict(c["theta"], c["lam"], (c["u"], c["v"], w), c["model"], ("wstack", c["opts"]))
    assert ctx.last_dropped() == 3 and np.all(out[bad] == 0) and rel(out, ref.predict(c["model"])) < TOL


def test_visibilities_at_the_grid_edge(ctx):
    """u, v up to +-0.5 lam and a little beyond: footprints cut by the grid's border, and some with no tap inside"""
    for N, msq in [(64, (4, 7, 4)), (65, (5, 9, 2))]:
        c = case(N, msq, 9, seed=31, span=0.56)
        ws = bind(ctx, c)
        e = [rel(host(ws.image(to_dev(c["vis"]))), c["image"]), rel(host(ws.predict(to_dev(c["model"]))), c["pred"])]
        print(N, e, "predict exactly 0:", int(np.sum(c["pred"] == 0)))
        # (a footprint wholly outside grids nothing and predicts 0, but is no "dropped" visibility: that counts w-bins
        # out of range, which a stack never has, and non-finite w)
        assert max(e) < TOL and np.any(c["pred"] == 0) and ws.dropped == 0
        ws.close()


# ---- 4: the adjoint identity on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,msq,L", [(64, (4, 7, 4), 9), (65, (3, 7, 1), 16)])
def test_adjoint_identity(ctx, N, msq, L):
    c = case(N, msq, L)
    ws = bind(ctx, c)
    lhs = np.sum(c["model"] * host(ws.image(to_dev(c["vis"]))))
    rhs = np.real(np.vdot(c["vis"], host(ws.predict(to_dev(c["model"]))))) / (N * N)
    print(lhs, rhs)
    assert abs(lhs - rhs) <= TOL * max(abs(lhs), abs(rhs))
    ws.close()


# ---- 5: capture, and no allocation after the first call -------------------------------------------------------------------------
def test_an_image_pass_can_be_captured_into_a_graph(ctx):
    import torch
    c = case(65, (4, 7, 4), 9)
    ws = bind(ctx, c)
    dvis = to_dev(c["vis"])
    img = torch.zeros((65, 65), dtype=torch.float64, device="cuda:0")
    eager = host(ws.image(dvis)).copy()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ws.image(dvis, out=img)  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one linear chain: no parallel branches
        ws.image(dvis, out=img)
    torch.cuda.synchronize()
    img.fill_(7.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    e = rel(host(img), eager)
    print(e)
    assert e < TOL and rel(eager, c["image"]) < TOL and ctx.get_option("errors") == 0
    ws.close()


def test_a_second_pass_allocates_nothing(ctx):
    import torch
    c = case(64, (5, 9, 2), 16)
    ws = bind(ctx, c)
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = torch.zeros((64, 64), dtype=torch.float64, device="cuda:0")
    out = torch.zeros(NVIS, dtype=torch.complex128, device="cuda:0")
    ws.image(dvis, out=img), ws.predict(dmodel, vis_sub=dvis, out=out)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    ws.image(dvis, out=img), ws.predict(dmodel, vis_sub=dvis, out=out), ws.predict(dmodel, out=out)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    assert rel(host(img), c["image"]) < TOL and rel(host(out), c["pred"]) < TOL
    ws.close()


# ---- 6: refusals and limits -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx):
    import torch
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    c = case(64, (4, 7, 4), 9)
    theta, lam, n = c["theta"], c["lam"], NVIS
    du, dv, dw, dvis, dmodel = (to_dev(c[k]) for k in ("u", "v", "w", "vis", "model"))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(wstep=WSTEP, M=4, Q=4, ff=NPIXFF, S=7, theta=theta, lam=lam, n=n, u=p(du), v=p(dv), w=p(dw), st=1)
    order = ("wstep", "M", "Q", "ff", "S", "theta", "lam", "n", "u", "v", "w", "st")
    bads = [dict(wstep=0), dict(M=0), dict(M=-1), dict(S=17), dict(Q=0), dict(ff=5, S=5), dict(theta=0.0), dict(n=-1),
            dict(st=0), dict(u=None), dict(w=None)]
    ctx.synchronize()
    for bad in bads:
        a = [dict(good, **bad)[k] for k in order]
        ws = C.c_void_p(0x1234)
        assert lib.gridhip_wstack_create_dev(h, *a, C.byref(ws)) == _lib.EINVAL, bad
        assert not ws.value, bad  # a refused creation leaves *ws NULL
        img = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
        psf = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
        out = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
        pm = C.c_double(7.0)
        assert lib.gridhip_do_imaging_wstack_dev(h, *a, p(dvis), p(img), p(psf), C.byref(pm)) == _lib.EINVAL, bad
        assert lib.gridhip_predict_wstack_dev(h, *a[:7], p(dmodel), *a[7:], None, p(out)) == _lib.EINVAL, bad
        torch.cuda.synchronize()
        assert bool((img == 7).all()) and bool((psf == 7).all()) and bool((out == 7).all()) and pm.value == 7.0, bad
    a = [good[k] for k in order]
    img = torch.full((64, 64), 7.0, dtype=torch.float64, device="cuda:0")
    out = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
    pm = C.c_double(7.0)
    assert lib.gridhip_do_imaging_wstack_dev(h, *a, p(dvis), p(img), None, C.byref(pm)) == _lib.EINVAL  # no psf
    assert lib.gridhip_do_imaging_wstack_dev(h, *a, None, p(img), p(img), C.byref(pm)) == _lib.EINVAL   # no vis
    assert lib.gridhip_predict_wstack_dev(h, *a[:7], None, *a[7:], None, p(out)) == _lib.EINVAL         # no model
    # the host forms, through the binding: the library's own refusal (the binding's check is bypassed)
    hu, hv, hw = (np.ascontiguousarray(c[k]) for k in "uvw")
    himg, hout = np.full((64, 64), 7.0), np.full(n, 7.0 + 0j)
    hp = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    ha = [dict(good, M=0, u=hp(hu), v=hp(hv), w=hp(hw))[k] for k in order]
    assert lib.gridhip_do_imaging_wstack(h, *ha, hp(c["vis"]), hp(himg), hp(himg), C.byref(pm)) == _lib.EINVAL
    assert lib.gridhip_predict_wstack(h, *ha[:7], hp(c["model"]), *ha[7:], None, hp(hout)) == _lib.EINVAL
    # the handle's passes
    ws = bind(ctx, c)
    assert lib.gridhip_wstack_image_dev(ws._h, None, p(img)) == _lib.EINVAL
    assert lib.gridhip_wstack_image_dev(ws._h, p(dvis), None) == _lib.EINVAL
    assert lib.gridhip_wstack_predict_dev(ws._h, None, None, p(out)) == _lib.EINVAL
    assert lib.gridhip_wstack_predict_dev(ws._h, p(dmodel), None, None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((img == 7).all()) and bool((out == 7).all()) and np.all(himg == 7) and np.all(hout == 7) and pm.value == 7.0
    ws.close()


def test_too_many_layers_is_unsupported_and_an_empty_stream_is_a_zero_image(ctx):
    import torch
    import gridhip
    from gridhip import _lib
    theta, lam = SHAPES[48]
    rng = np.random.default_rng(41)
    n = 64
    u, v = rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)
    w = rng.uniform(-1000, 1000, n)
    w[0], w[1] = 0.0, 4096.0 * WSTEP  # planes 0 .. 4096 with M = 1: 4097 layers
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.wstack(theta, lam, tuple(to_dev(x) for x in (u, v, w)), opts(1, 7, 2))
    assert ei.value.code == _lib.EUNSUPPORTED
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.predict(theta, lam, (u, v, w), np.zeros((48, 48)), ("wstack", opts(1, 7, 2)))
    assert ei.value.code == _lib.EUNSUPPORTED
    w[1] = 4095.0 * WSTEP  # planes 0 and 4095, everything else in plane 0: 4096 layers, the limit, two of them occupied
    ws = ctx.wstack(theta, lam, tuple(to_dev(x) for x in (u, v, np.where(np.arange(n) < 2, w, 0.0))), opts(1, 7, 2))
    assert (ws.layers, ws.occupied) == (4096, 2)
    ws.close()
    # n = 0: L = 0, a zero image, no error
    e = torch.zeros(0, dtype=torch.float64, device="cuda:0")
    ws = ctx.wstack(theta, lam, (e, e, e), opts(3, 7, 2))
    img = torch.full((48, 48), 7.0, dtype=torch.float64, device="cuda:0")
    ws.image(torch.zeros(0, dtype=torch.complex128, device="cuda:0"), out=img)
    assert (ws.layers, ws.occupied, ws.dropped) == (0, 0, 0) and not bool(img.any())
    assert ws.predict(torch.zeros((48, 48), dtype=torch.float64, device="cuda:0")).shape == (0,)
    ws.close()
