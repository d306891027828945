"""The aw imaging entry points: gridhip_aw_imaging_dev, gridhip_do_imaging_aw[_dev] (do_imaging with
imgfn = aw_imaging, src/Gridding.hs:509-549) and gridhip_aw_gridding[_dev] (src/ImageDataset.hs:54-77 as one call),
against the CPU oracle and against the composition of the older single-step calls."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import gridref_np as P

pytestmark = pytest.mark.gpu
C_LIGHT = 299792458.0


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def tables(W, Q, S, A, wmax, seed):
    rng = np.random.default_rng(seed)
    wk = (rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))) / S
    # A-kernels with no symmetry: a[i, j] != a[S-1-i, S-1-j]
    ak = (rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))) / S + np.linspace(0, 1, S)[None, :, None]
    assert not np.allclose(ak[0], ak[0][::-1, ::-1])
    return wk, np.linspace(-wmax, wmax, W), ak


def stream(n, lam, A, wmax, seed, span=0.45):
    """uvw in wavelengths, v of both signs, w a little beyond the outer planes (findClosest clamps)"""
    rng = np.random.default_rng(seed)
    uvw = np.stack([rng.uniform(-span, span, n) * lam, rng.uniform(-span, span, n) * lam,
                    rng.uniform(-1.1 * wmax, 1.1 * wmax, n)], axis=1)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    return uvw, rng.integers(0, A, n), rng.integers(0, A, n), vis


def oracle_imgfn(oracle, wk, wv, ak, a1, a2):
    """aw_imaging (:452-478) through the C oracle: p = uvw / lam, findClosest of w, convgrid4"""
    def imgfn(theta, lam, u1, v1, w1, vs):
        N = P.haskell_round(theta * lam)
        wb = np.array([oracle.find_closest(wv, x) for x in w1], dtype=np.int64)
        return oracle.awgrid(wk, ak, np.zeros((N, N), dtype=np.complex128), u1 / np.float64(lam),
                             v1 / np.float64(lam), wb, a1, a2, vs)
    return imgfn


def oracle_aw_gridding(oracle, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis, weigh_mirrored=False):
    """the chain of tests/test_h5io.py (src/ImageDataset.hs:54-77); weigh_mirrored: the other doweight order"""
    p = uvw_m * (f / C_LIGHT)  # uvw_lambda, src/ImageDataset.hs:181-187
    N = P.haskell_round(theta * lam)
    u1, v1, w1, vis1 = P.mirror_uvw(p[:, 0], p[:, 1], p[:, 2], vis)
    if weigh_mirrored:
        wt = P.doweight(N, u1 / lam, v1 / lam, np.ones(len(vis), dtype=np.complex128))
    else:
        wt = P.doweight(N, p[:, 0] / lam, p[:, 1] / lam, np.ones(len(vis), dtype=np.complex128))
    G = oracle_imgfn(oracle, wk, wv, ak, a1, a2)(theta, lam, u1, v1, w1, vis1 * wt)
    return np.real(P.ifft_c(P.make_grid_hermitian(G)))


def test_do_imaging_aw_matches_oracle_at_driver_size(ctx, oracle):
    theta, lam, W, Q, S, A, n = 0.008, 300000, 9, 4, 15, 6, 20000
    wk, wv, ak = tables(W, Q, S, A, 400.0, 1)
    uvw, a1, a2, vis = stream(n, lam, A, 400.0, 2)
    assert (uvw[:, 1] < 0).any() and (uvw[:, 1] > 0).any()
    img, psf, pmax = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", wk, wv, ak))
    assert img.shape == (2400, 2400)
    ri, rp, rm = P.do_imaging(theta, lam, uvw[:, 0], uvw[:, 1], uvw[:, 2], vis, oracle_imgfn(oracle, wk, wv, ak, a1, a2))
    assert rel(img, ri) < 1e-10
    assert rel(psf, rp) < 1e-10
    assert abs(pmax - rm) <= 1e-10 * abs(rm)
    assert abs(psf.max() - 1.0) < 1e-12


def test_do_imaging_aw_resident_form(ctx):
    import torch
    theta, lam, W, Q, S, A, n = 0.008, 12000, 5, 2, 9, 5, 30000  # N = 96
    wk, wv, ak = tables(W, Q, S, A, 300.0, 3)
    uvw, a1, a2, vis = stream(n, lam, A, 300.0, 4)
    img, psf, pmax = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", wk, wv, ak))
    dev = torch.device("cuda:0")
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (uvw, a1, a2, vis, wk, wv, ak)]
    keep = [x.clone() for x in d]
    for _ in range(2):  # the second call runs from the context's pool
        dimg, dpsf, dpmax = ctx.do_imaging(theta, lam, d[0], d[1], d[2], None, None, d[3], ("aw", d[4], d[5], d[6]))
        assert dimg.is_cuda and dpsf.is_cuda
        assert rel(dimg.cpu().numpy(), img) < 1e-12
        assert rel(dpsf.cpu().numpy(), psf) < 1e-12
        assert abs(dpmax - pmax) <= 1e-12 * abs(pmax)
    for x, k in zip(d, keep):
        assert torch.equal(x, k)  # inputs unmodified


def five_call_aw_gridding(ctx, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis):
    """the Python composition python/gridhip/dataset.py used before gridhip_aw_gridding existed"""
    uvw0 = uvw_m * (f / C_LIGHT)
    cols = (uvw0[:, 0].copy(), uvw0[:, 1].copy(), uvw0[:, 2].copy())
    wt = ctx.doweight(theta, lam, cols, np.ones(len(vis), dtype=np.complex128))
    uvw1, vis1 = ctx.mirror_uvw(cols, vis)
    g = ctx.aw_imaging(theta, lam, wk, wv, ak, uvw1, (a1, a2, None, f), vis1 * wt)
    return np.real(ctx.ifft(ctx.make_grid_hermitian(g)))


@pytest.mark.parametrize("lam,n", [(8000, 3000), (300000, 4000)])  # N = 64, N = 2400
def test_aw_gridding_one_call_matches_oracle_chain(ctx, oracle, lam, n):
    import torch
    theta, f, W, Q, S, A = 0.008, 1.0e8, 5, 2, 15, 4
    wk, wv, ak = tables(W, Q, S, A, 200.0, 5)
    uvw, a1, a2, vis = stream(n, lam, A, 200.0, 6, span=0.4)
    uvw_m = np.ascontiguousarray(uvw * (C_LIGHT / f))  # metres, as /vis/uvw stores them
    img, mx = ctx.aw_gridding(theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis)
    ref = oracle_aw_gridding(oracle, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis)
    assert rel(img, ref) < 1e-10
    assert abs(mx - ref.max()) <= 1e-10 * abs(ref.max())
    assert mx == img.max()
    old = five_call_aw_gridding(ctx, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis)
    assert rel(img, old) < 1e-12
    # the resident form, uvw as the (n, 3) matrix
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dimg, dmx = ctx.aw_gridding(theta, lam, f, t(wk), t(wv), t(ak), t(uvw_m), t(a1), t(a2), t(vis))
    assert rel(dimg.cpu().numpy(), img) < 1e-12 and abs(dmx - mx) <= 1e-12 * abs(mx)


def test_doweight_order_is_pinned_per_entry_point(ctx, oracle):
    """(u, v) and (-u, -v): one cell after the mirror, two before.  do_imaging weighs the mirrored uvw (each 1/2),
    aw_gridding the un-mirrored one (each 1)."""
    theta, lam, f, W, Q, S, A = 0.008, 8000, 1.0e8, 3, 2, 7, 3
    N = 64
    wk, wv, ak = tables(W, Q, S, A, 100.0, 7)
    uvw = np.array([[0.1 * lam, 0.2 * lam, 30.0], [-0.1 * lam, -0.2 * lam, -30.0]])
    x = np.floor(0.5 + N // 2 + N * uvw[:, 0] / lam)
    assert x[0] != x[1]
    a1, a2 = np.array([0, 1]), np.array([2, 0])
    vis = np.array([1.0 + 0.5j, -0.3 + 0.8j])
    # do_imaging: the weights are 1/2, so the PSF's peak is that of two visibilities of weight 1/2 each
    img, psf, pmax = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", wk, wv, ak))
    imgfn = oracle_imgfn(oracle, wk, wv, ak, a1, a2)
    ri, rp, rm = P.do_imaging(theta, lam, uvw[:, 0], uvw[:, 1], uvw[:, 2], vis, imgfn)
    assert rel(img, ri) < 1e-10 and rel(psf, rp) < 1e-10 and abs(pmax - rm) <= 1e-10 * abs(rm)
    u1, v1, w1, vis1 = P.mirror_uvw(uvw[:, 0], uvw[:, 1], uvw[:, 2], vis)
    psf_w1 = np.real(P.ifft_c(P.make_grid_hermitian(imgfn(theta, lam, u1, v1, w1, np.ones(2, dtype=np.complex128)))))
    assert abs(pmax - 0.5 * psf_w1.max()) <= 1e-10 * abs(pmax)  # each weighted by 1/2, not by 1
    # aw_gridding: weights from the un-mirrored uvw, two cells, 1 each
    uvw_m = uvw * (C_LIGHT / f)
    gimg, gmx = ctx.aw_gridding(theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis)
    ref = oracle_aw_gridding(oracle, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis)
    wrong = oracle_aw_gridding(oracle, theta, lam, f, wk, wv, ak, uvw_m, a1, a2, vis, weigh_mirrored=True)
    assert rel(gimg, ref) < 1e-10 and abs(gmx - ref.max()) <= 1e-10 * abs(ref.max())
    assert rel(wrong, ref) > 0.4  # (the other order halves everything)


def test_mirror_keeps_antenna_order(ctx, oracle):
    """A single visibility with v < 0, a1 != a2, A-kernels without symmetry.  The mirror negates uvw and conjugates
    vis only (:551-562): the antennas reach the gridder in the given order.  (aw_kernel_fn2 convolves the two A-kernels,
    and convolve2d commutes, so a swapped pair would build the same kernel - the swap is pinned here by matching the
    given order and checking that symmetry, not by a difference in the grid.)"""
    import torch
    theta, lam, W, Q, S, A = 0.008, 8000, 3, 2, 9, 4
    N = 64
    wk, wv, ak = tables(W, Q, S, A, 100.0, 9)
    uvw = np.array([[0.13 * lam, -0.21 * lam, -40.0]])
    a1, a2, vis = np.array([3]), np.array([1]), np.array([0.7 - 0.4j])
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    g = ctx.aw_imaging(theta, lam, t(wk), t(wv), t(ak), t(uvw), (t(a1), t(a2), None, None), t(vis)).cpu().numpy()
    ref = oracle_imgfn(oracle, wk, wv, ak, a1, a2)(theta, lam, uvw[:, 0], uvw[:, 1], uvw[:, 2], vis)
    assert rel(g, ref) < 1e-10
    swapped = oracle_imgfn(oracle, wk, wv, ak, a2, a1)(theta, lam, uvw[:, 0], uvw[:, 1], uvw[:, 2], vis)
    assert rel(swapped, ref) < 1e-12  # convolve2d(a, b) == convolve2d(b, a)
    # through do_imaging's mirror: matches the oracle with the antennas as given
    img, psf, pmax = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", wk, wv, ak))
    ri, rp, rm = P.do_imaging(theta, lam, uvw[:, 0], uvw[:, 1], uvw[:, 2], vis, oracle_imgfn(oracle, wk, wv, ak, a1, a2))
    assert rel(img, ri) < 1e-10 and rel(psf, rp) < 1e-10 and abs(pmax - rm) <= 1e-10 * abs(rm)


def naive_do_imaging(ctx, theta, lam, uvw, a1, a2, vis, wk, wv, ak):
    """do_imaging composed from the single-step calls: mirror, doweight, two aw_imaging_dev calls, hermitian, ifft"""
    import torch
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    N = ctx.image_size(theta, lam)
    uvw1, vis1 = ctx.mirror_uvw((uvw[:, 0], uvw[:, 1], uvw[:, 2]), vis)
    wt = ctx.doweight(theta, lam, uvw1, np.ones(len(vis), dtype=np.complex128))
    duvw = t(np.stack(uvw1, axis=1))
    built = []
    out = []
    for vs in (wt * vis1, wt):
        g = ctx.aw_imaging(theta, lam, t(wk), t(wv), t(ak), duvw, (t(a1), t(a2), None, None), t(vs)).cpu().numpy()
        built.append((ctx.get_option("aw_tables_built"), ctx.aw_stats()["kernels_built"]))
        out.append(np.real(ctx.ifft(ctx.make_grid_hermitian(g))))
    pmax = out[1].max()
    return out[0] / pmax, out[1] / pmax, pmax, built


@pytest.mark.parametrize("n", [200_000, 1_500_000])
def test_one_table_build_per_batch(ctx, n):
    import torch
    theta, lam, W, Q, S, A = 0.008, 64000, 4, 2, 9, 8  # N = 512
    wk, wv, ak = tables(W, Q, S, A, 300.0, 11)
    uvw, a1, a2, vis = stream(n, lam, A, 300.0, 12)
    bad = np.arange(37) * (n // 37)
    a1[bad] = A  # out of range: dropped and counted
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    img, psf, pmax = ctx.do_imaging(theta, lam, t(uvw), t(a1), t(a2), None, None, t(vis), ("aw", t(wk), t(wv), t(ak)))
    assert ctx.get_option("aw_tables_built") == math.ceil(n / 2 ** 20)
    assert ctx.get_option("errors") == 0
    assert ctx.last_dropped() == len(bad)
    kb = ctx.aw_stats()["kernels_built"]
    ni, npsf, npmax, built = naive_do_imaging(ctx, theta, lam, uvw, a1, a2, vis, wk, wv, ak)
    assert built[0] == built[1] == (math.ceil(n / 2 ** 20), kb)  # each naive pass builds what the one call built once
    assert rel(img.cpu().numpy(), ni) < 1e-12
    assert rel(psf.cpu().numpy(), npsf) < 1e-12
    assert abs(pmax - npmax) <= 1e-12 * abs(npmax)


def test_argument_checks(ctx):
    from gridhip import _lib
    lib = ctx._lib
    theta, lam, W, Q, S, A, n = 0.008, 8000, 2, 2, 5, 2, 4
    wk, wv, ak = tables(W, Q, S, A, 10.0, 13)
    uvw, a1, a2, vis = stream(n, lam, A, 10.0, 14)
    u, v, w = (np.ascontiguousarray(uvw[:, i]) for i in range(3))
    p = lambda x: C.c_void_p(x.ctypes.data)
    N = 64
    img, psf = np.full((N, N), 7.0), np.full((N, N), 7.0)
    grid = np.full((N, N), 7.0 + 0j)
    mx = C.c_double(7.0)

    def args(**kw):
        a = dict(theta=theta, lam=lam, W=W, Q=Q, S=S, A=A, wk=p(wk), wv=p(wv), ak=p(ak), n=n, u=p(u), v=p(v), w=p(w),
                 st=1, a1=p(a1), a2=p(a2), vis=p(vis))
        a.update(kw)
        return a

    def do(fn, a, outs):
        head = [ctx._h, a["theta"], a["lam"]]
        if "gridding" in fn:
            head.append(1.0e8)
        return getattr(lib, fn)(*head, a["W"], a["Q"], a["S"], a["A"], a["wk"], a["wv"], a["ak"], a["n"], a["u"],
                                a["v"], a["w"], a["st"], a["a1"], a["a2"], a["vis"], *outs)

    cases = [dict(wk=None), dict(wv=None), dict(ak=None), dict(u=None), dict(w=None), dict(a1=None), dict(a2=None),
             dict(vis=None), dict(S=0), dict(S=-3), dict(A=0), dict(A=-1), dict(theta=1e-6), dict(lam=0)]
    for kw in cases:
        a = args(**kw)
        assert do("gridhip_do_imaging_aw", a, [p(img), p(psf), C.byref(mx)]) == _lib.EINVAL, kw
        assert do("gridhip_aw_gridding", a, [p(img), C.byref(mx)]) == _lib.EINVAL, kw
    assert do("gridhip_do_imaging_aw", args(), [None, p(psf), C.byref(mx)]) == _lib.EINVAL
    assert do("gridhip_do_imaging_aw", args(), [p(img), None, C.byref(mx)]) == _lib.EINVAL
    assert do("gridhip_aw_gridding", args(), [None, C.byref(mx)]) == _lib.EINVAL
    assert (img == 7.0).all() and (psf == 7.0).all() and mx.value == 7.0
    # the resident forms check the same before touching a device pointer (null / S / A / N)
    import torch
    dgrid = torch.full((N, N), 7.0 + 0j, dtype=torch.complex128, device="cuda:0")
    dimg = torch.full((N, N), 7.0, dtype=torch.float64, device="cuda:0")
    dp = lambda x: C.c_void_p(x.data_ptr())
    for kw in (dict(wk=None), dict(S=0), dict(A=0), dict(theta=1e-6)):
        a = args(**kw)
        assert do("gridhip_aw_imaging_dev", a, [dp(dgrid)]) == _lib.EINVAL, kw
        assert do("gridhip_do_imaging_aw_dev", a, [dp(dimg), dp(dimg), C.byref(mx)]) == _lib.EINVAL, kw
        assert do("gridhip_aw_gridding_dev", a, [dp(dimg), C.byref(mx)]) == _lib.EINVAL, kw
    assert do("gridhip_aw_imaging_dev", args(), [None]) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((dgrid == 7.0).all()) and bool((dimg == 7.0).all()) and mx.value == 7.0
    assert (grid == 7.0).all()
