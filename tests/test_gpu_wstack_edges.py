"""W-stacking on the device (wstack.hip, idg.hip) at the inputs the seeded streams of test_gpu_wstack.py,
test_gpu_wstack_imager.py and test_gpu_idg.py never reach: w on exact plane ties, streams that take more than one
work-group of the scatter and more layers than the scan has threads, fields wide enough for screens of hundreds of turns,
subgrids and images that reach past the horizon, every width of the image-domain degridder, and degenerate streams.
The cases and their preconditions are tests/wstack_edge_cases.py and tests/test_wstack_edges_host.py.

Tolerances are the project's own, none is measured here.  W-projection stacks: 1e-10 of the reference's largest
magnitude (TOL of test_gpu_wstack.py).  Image-domain layers: image_tol and predict_tol of test_gpu_idg.py, per element;
their premise, phases below 100 turns, is asserted case by case by the host test.  layers, occupied, pmin, dropped and
last_dropped() are compared exactly; a dropped visibility's prediction is +0 and its residual `vis`, bit for bit.

Every case goes through a handle: image, predict, predict(vis_sub=) and a second image (the grid is clear again); where
noted also through the one-call do_imaging / predict in the device form, and through an imager."""
import ctypes as C

import numpy as np
import pytest

import wstack_edge_cases as E
from test_gpu_idg import bits, image_tol, predict_tol, within
from test_gpu_wstack import TOL, host, rel
from test_gpu_wstack_imager import against_the_calls

pytestmark = pytest.mark.gpu


def to_dev(x):
    """a device copy (the cases' arrays are read-only, and stay as they are)"""
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")


def dev3(c):
    return tuple(to_dev(c[k]) for k in "uvw")


def close_to(c, what, got, ref):
    """the file's tolerance for the case's kind: relative to the largest magnitude, or per element"""
    if c["fn"][0] == "wstack":
        e = rel(got, ref)
        print(f"  {what}: {e:.2e}")
        assert np.isfinite(got).all() and e < TOL, f"{what}: {e}"
    else:
        N, K = c["N"], c["fn"][1]["margin"]
        tol = image_tol(N, K, np.abs(c["vis"]).sum() / N ** 2) if got.ndim == 2 else predict_tol(N, K, c["model"])
        within(got, ref, tol, what)


def handle(ctx, c, what):
    """the integers, then image, predict, the residual and the image again through a stack handle"""
    ref = c["ref"]
    print(f"{what}: N={c['N']} n={c['n']} {c['fn'][1]} layers {ref.lay['L']} occupied {len(ref.occupied)}")
    ws = ctx.wstack(c["theta"], c["lam"], dev3(c), c["fn"])
    assert (ws.layers, ws.occupied, ws.pmin, ws.dropped) == (ref.lay["L"], len(ref.occupied), ref.lay["pmin"], c["dropped"])
    assert ctx.last_dropped() == c["dropped"]
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = host(ws.image(dvis))
    pred = host(ws.predict(dmodel))
    res = host(ws.predict(dmodel, vis_sub=dvis))
    img2 = host(ws.image(dvis))
    assert ctx.last_dropped() == c["dropped"]
    ws.close()
    close_to(c, "image", img, c["image"])
    close_to(c, "predict", pred, c["pred"])
    close_to(c, "residual", res, c["vis"] - c["pred"])
    close_to(c, "image again", img2, c["image"])
    gone = ~c["kept"]
    assert np.all(bits(pred)[gone] == 0) and np.array_equal(bits(res)[gone], bits(c["vis"])[gone])
    assert ctx.get_option("errors") == 0
    return img, pred


def calls(ctx, c, ref_imaging):
    """the one-call forms of a w-projection stack on device arrays: do_imaging (whose mirror negates w where v < 0),
    predict and predict(vis_sub=)"""
    r_img, r_psf, r_pmax = ref_imaging
    img, psf, pmax = ctx.do_imaging(c["theta"], c["lam"], dev3(c), None, None, None, None, to_dev(c["vis"]), c["fn"])
    close_to(c, "do_imaging image", host(img), r_img)
    close_to(c, "do_imaging psf", host(psf), r_psf)
    assert abs(pmax - r_pmax) < TOL * r_pmax
    dmodel, dsub = to_dev(c["model"]), to_dev(c["vis"])
    close_to(c, "predict, one call", host(ctx.predict(c["theta"], c["lam"], dev3(c), dmodel, c["fn"])), c["pred"])
    assert ctx.last_dropped() == c["dropped"]
    close_to(c, "residual, one call", host(ctx.predict(c["theta"], c["lam"], dev3(c), dmodel, c["fn"], vis_sub=dsub)),
             c["vis"] - c["pred"])
    assert ctx.get_option("errors") == 0


def adjoint(ctx, c, tol):
    """test_adjoint_identity of test_gpu_wstack.py / test_gpu_idg.py on a case"""
    N = c["N"]
    ws = ctx.wstack(c["theta"], c["lam"], dev3(c), c["fn"])
    lhs = np.sum(c["model"] * host(ws.image(to_dev(c["vis"]))))
    rhs = np.real(np.vdot(c["vis"], host(ws.predict(to_dev(c["model"]))))) / (N * N)
    ws.close()
    print(f"  adjoint: {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= tol * max(abs(lhs), abs(rhs))


# ---- T: plane ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3])
def test_ties(ctx, M):
    """every w on a half-plane: libm round, away from zero.  do_imaging's mirror negates w, so its stack meets the ties
    of the other sign as well."""
    c = E.ties(M)
    assert c["ref"].lay["pmin"] == -7
    handle(ctx, c, f"ties, M = {M}")
    mirrored = np.where(c["v"] < 0, -c["w"], c["w"])
    assert (mirrored[c["v"] < 0] > 0).any() and (mirrored[c["v"] < 0] < 0).any()
    calls(ctx, c, E.imaging(E.ties, M))


def test_ties_through_image_domain_layers(ctx):
    handle(ctx, E.ties_idg(), "ties, image-domain layers")


# ---- S: the scatter's seams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msq", E.SEAM_MSQ, ids=lambda x: "M%d-S%d-Q%d" % x)
@pytest.mark.parametrize("n", E.SEAM_N)
def test_scatter_seams(ctx, n, msq):
    handle(ctx, E.seam(n, msq), f"{-(-n // E.SCATTER)} work-group(s) of the scatter")


def test_scatter_seams_one_plane(ctx):
    handle(ctx, E.one_plane(), "every work-group adds to one cursor")


def test_scatter_seams_every_layer(ctx):
    handle(ctx, E.every_layer(), "every work-group adds to every cursor")


def test_scatter_seams_under_an_imager(ctx):
    """the imager's compose and middle kernels over slices that several work-groups filled"""
    N, msq, L, n = E.IMAGER_SEAM
    against_the_calls(ctx, N, msq, L, n=n)


# ---- C: the scan's seams --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [257, 515])
def test_scan_seams(ctx, L):
    c = E.scan(L)
    assert c["ref"].lay["L"] == L and len(c["ref"].occupied) == len(E.scan_occupied(L))
    handle(ctx, c, f"{-(-L // E.SCAN)} layers per thread of the scan")


# ---- F: wide fields -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [48, 65])
def test_wide_fields(ctx, N):
    c = E.wide(N)
    handle(ctx, c, f"screens of {E.screen_turns(c):.0f} turns")
    calls(ctx, c, E.imaging(E.wide, N))
    if N == 65:
        adjoint(ctx, c, TOL)


# ---- D: degenerate streams and the limit ----------------------------------------------------------------------------------
def test_one_visibility(ctx):
    c = E.one_visibility()
    handle(ctx, c, "one visibility")
    calls(ctx, c, E.imaging(E.one_visibility))


def test_no_finite_w(ctx):
    import torch
    c = E.no_finite_w()
    n, N = c["n"], c["N"]
    ws = ctx.wstack(c["theta"], c["lam"], dev3(c), c["fn"])
    assert (ws.layers, ws.occupied, ws.dropped) == (0, 0, n) and ctx.last_dropped() == n
    dvis, dmodel = to_dev(c["vis"]), to_dev(c["model"])
    img = torch.full((N, N), 7.0, dtype=torch.float64, device="cuda:0")
    assert ws.image(dvis, out=img) is img
    assert not bits(host(img)).any()  # exactly +0 everywhere
    pred = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
    ws.predict(dmodel, out=pred)
    assert not bits(host(pred)).any()
    assert np.array_equal(bits(host(ws.predict(dmodel, vis_sub=dvis))), bits(c["vis"]))
    buf = dvis.clone()
    assert ws.predict(dmodel, vis_sub=buf, out=buf) is buf and np.array_equal(bits(host(buf)), bits(c["vis"]))
    ws.close()
    # the one-call forms
    out = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
    ctx.predict(c["theta"], c["lam"], dev3(c), dmodel, c["fn"], out=out)
    assert not bits(host(out)).any() and ctx.last_dropped() == n
    res = host(ctx.predict(c["theta"], c["lam"], dev3(c), dmodel, c["fn"], vis_sub=dvis))
    assert np.array_equal(bits(res), bits(c["vis"])) and ctx.last_dropped() == n
    hres = ctx.predict(c["theta"], c["lam"], tuple(c[k].copy() for k in "uvw"), c["model"].copy(), c["fn"],
                       vis_sub=c["vis"].copy())
    assert np.array_equal(bits(hres), bits(c["vis"]))
    # do_imaging: a zero image and a zero psf, divided by the psf's maximum 0, as the restatement's
    r_img, r_psf, r_pmax = E.imaging(E.no_finite_w)
    img, psf, pmax = ctx.do_imaging(c["theta"], c["lam"], dev3(c), None, None, None, None, dvis, c["fn"])
    assert ctx.last_dropped() == n and pmax == r_pmax == 0.0
    assert np.array_equal(host(img), r_img, equal_nan=True) and np.array_equal(host(psf), r_psf, equal_nan=True)
    assert ctx.get_option("errors") == 0


def test_the_plane_limit(ctx):
    """wstep = 1: a plane of 2^52 + 2 is refused as unsupported, with *ws NULL and the outputs untouched; 2^52 is taken"""
    import torch
    import gridhip
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    theta, lam, N, n = E.THETA48, E.LAM48, 48, 6
    rng = np.random.default_rng(520)
    u, v = E.uv(rng, n, lam)
    du, dv = to_dev(u), to_dev(v)
    dvis, dmodel = to_dev(rng.normal(size=n) + 0j), to_dev(rng.normal(size=(N, N)))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    big = E.TWO52 + 2.0
    fn = E.wfn(1, 7, 2, wstep=1)
    for w in (np.full(n, big), np.full(n, -big), np.where(np.arange(n) % 2 == 0, big, -big),
              np.where(np.arange(n) == 3, big, 0.0)):
        dw = to_dev(w)
        ctx.synchronize()
        a = (1, 1, 2, E.NPIXFF, 7, theta, lam, n, p(du), p(dv), p(dw), 1)
        ws = C.c_void_p(0x1234)
        assert lib.gridhip_wstack_create_dev(h, *a, C.byref(ws)) == _lib.EUNSUPPORTED
        assert not ws.value
        img = torch.full((N, N), 7.0, dtype=torch.float64, device="cuda:0")
        psf = torch.full((N, N), 7.0, dtype=torch.float64, device="cuda:0")
        out = torch.full((n,), 7.0, dtype=torch.complex128, device="cuda:0")
        pm = C.c_double(7.0)
        assert lib.gridhip_do_imaging_wstack_dev(h, *a, p(dvis), p(img), p(psf), C.byref(pm)) == _lib.EUNSUPPORTED
        assert lib.gridhip_predict_wstack_dev(h, *a[:7], p(dmodel), *a[7:], None, p(out)) == _lib.EUNSUPPORTED
        torch.cuda.synchronize()
        assert bool((img == 7).all()) and bool((psf == 7).all()) and bool((out == 7).all()) and pm.value == 7.0
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.wstack(theta, lam, (du, dv, dw), fn)
        assert ei.value.code == _lib.EUNSUPPORTED
    for sign in (1.0, -1.0):
        ws = ctx.wstack(theta, lam, (du, dv, to_dev(np.full(n, sign * E.TWO52))), fn)
        assert (ws.layers, ws.occupied, ws.pmin, ws.dropped) == (1, 1, int(sign) * 2 ** 52, 0)
        ws.close()


# ---- H: the horizon (image-domain layers) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", E.SUBGRIDS, ids=str)
def test_horizon(ctx, sk):
    c = E.horizon(sk)
    img, _ = handle(ctx, c, f"theta = {c['theta']}")
    out = E.beyond(c)
    assert out.any() and not bits(img)[out].any()  # exactly +0 on every cell on or beyond the horizon
    adjoint(ctx, c, 1e-9)


# ---- G: the degridder's widths (image-domain layers) ----------------------------------------------------------------------
@pytest.mark.parametrize("n", E.WIDTH_N)
@pytest.mark.parametrize("sk", E.SUBGRIDS, ids=str)
def test_degridder_widths(ctx, sk, n):
    assert ctx.get_option("idg_split") == E.SPLIT
    c = E.width(sk, n)
    (tiles, nitems, nvis), = E.items(c)
    handle(ctx, c, f"one tile of {n}: {nitems} item(s), {E.degrid_threads(nvis // nitems)} threads")


@pytest.mark.parametrize("sk", E.SUBGRIDS, ids=str)
def test_a_full_item_under_the_narrow_launch(ctx, sk):
    assert ctx.get_option("idg_split") == E.SPLIT
    c = E.mixed(sk)
    (tiles, nitems, nvis), = E.items(c)
    assert E.degrid_threads(nvis // nitems) == 64
    handle(ctx, c, f"{tiles} tiles, {nitems} items, mean {nvis // nitems}")
