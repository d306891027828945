"""Imagers on the GPU (gridhip_imager_*, Context.imager): an imager against the two calls it replaces on the same device,
against numpy (oracle/gridref_np's do_imaging composed with a restatement of the prediction), linearity, isolation from
every other call on the context, driver size, several aw batches, capture into a graph, refusals and edges.
Tolerances are the project's own: 1e-10 of the reference output's largest magnitude (the fp64 atomics make neither side
bit-reproducible), 1e-12 relative for pmax and for an imager against itself."""
import ctypes as C

import numpy as np
import pytest

from oracle import gridref_np as P

pytestmark = pytest.mark.gpu

KO = {"wstep": 40, "qpx": 2, "npixFF": 16, "npixKern": 7}
SHAPES = [(0.1, 640), (0.1, 490)]  # N = 64 (even) and N = 49 (odd)
KINDS = ["simple", "conv", "w_cache", "aw"]
A = 4  # antennas of the aw tables


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- test_gpu_predict.py's generators, restated ---------------------------------------------------------------------
def stream(n, lam, wmax, seed, span=0.55, nans=False):
    """uvw in wavelengths (some beyond the grid's edge), vis"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-span, span, n) * lam
    v = rng.uniform(-span, span, n) * lam
    w = rng.uniform(-wmax, wmax, n)
    if nans:
        u[3], v[5] = np.nan, np.nan
    return u, v, w, rng.normal(size=n) + 1j * rng.normal(size=n)


def aw_tables(W, Q, S, A, wmax, seed):
    rng = np.random.default_rng(seed)
    wk = (rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))) / S
    ak = (rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))) / S + np.linspace(0, 1, S)[None, :, None]
    return wk, np.linspace(-wmax, wmax, W), ak


def kv_table(Q, S, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(Q, Q, S, S)) + 1j * rng.normal(size=(Q, Q, S, S))


def setup(kind, theta, lam, n, seed, nans=False, bad_antennas=True):
    """simple: NaN coordinates; aw: antennas out of range (findClosest always returns a w-bin inside the table, so an
    out-of-range w-bin cannot be given through the imaging interface)"""
    N = P.haskell_round(theta * lam)
    u, v, w, vis = stream(n, lam, 100.0, seed, nans=nans)
    rng = np.random.default_rng(seed + 1)
    model = rng.normal(size=(N, N))
    kv = kv_table(4, 7, seed) if kind == "conv" else None
    aw = None
    if kind == "aw":
        wk, wv, ak = aw_tables(3, 2, 9, A, 100.0, seed)
        a1, a2 = rng.integers(0, A, n), rng.integers(0, A, n)
        if bad_antennas and n > 20:
            a1[2], a2[11], a1[17] = A, -1, A + 5
        aw = (wk, wv, ak, a1, a2)
    return N, (u, v, w), vis, model, kv, aw


def imgfn_of(kind, kv=None, aw=None, ko=KO):
    if kind == "simple":
        return ("simple",)
    if kind == "conv":
        return ("conv", kv)
    if kind == "w_cache":
        return ("w_cache", ko)
    return ("aw", aw[0], aw[1], aw[2])


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


# ---- numpy: the prediction (restate of test_gpu_predict.py) and the imaging functions do_imaging is composed with ------
def aw_kernel(cache, wk, wv, ak, w, a1, a2, yf, xf):
    wb = P.find_closest(wv, w)
    key = (wb, a1, a2, yf, xf)
    if key not in cache:
        cache[key] = P.aw_kernel_fn2(yf, xf, wk[wb], ak[a1], ak[a2])
    return cache[key]


def restate(kind, theta, lam, model, u, v, w, kv=None, ko=None, aw=None):
    """pred = A^H fft_c(model); aw = (wk, wvals, ak, a1, a2)"""
    N = model.shape[0]
    F = P.fft_c(model.astype(np.complex128))
    pu, pv = u / np.float64(lam), v / np.float64(lam)
    if kind == "simple":
        out = np.zeros(len(u), dtype=np.complex128)
        ok = ~(np.isnan(pu) | np.isnan(pv))
        x = N // 2 + np.floor(0.5 + np.float64(N) * pu[ok]).astype(np.int64)
        y = N // 2 + np.floor(0.5 + np.float64(N) * pv[ok]).astype(np.int64)
        inside = (x >= 0) & (y >= 0) & (x < N) & (y < N)
        vals = np.zeros(ok.sum(), dtype=np.complex128)
        vals[inside] = F[y[inside], x[inside]]
        out[ok] = vals
        return out
    if kind == "conv":
        return P.degrid2(np.conj(kv)[None], F, pu, pv, np.zeros(len(u), dtype=np.int64))
    if kind == "w_cache":
        wb, wmin, steps = P.wbins(w, ko["wstep"])
        kerns = np.stack([P.w_kernel(theta, float(i * ko["wstep"] + wmin), ko["npixFF"], ko["npixKern"], ko["qpx"])
                          for i in range(steps)])
        return P.degrid2(kerns, F, pu, pv, wb)
    wk, wv, ak, a1, a2 = aw
    S = wk.shape[-1]
    x, xf, y, yf = P.frac_coords((N, N), wk.shape[1], pu, pv)
    out = np.zeros(len(u), dtype=np.complex128)
    cache = {}
    for k in range(len(u)):
        if not (0 <= a1[k] < len(ak) and 0 <= a2[k] < len(ak)):
            continue
        kern = aw_kernel(cache, wk, wv, ak, w[k], a1[k], a2[k], yf[k], xf[k])
        ys, xs = np.arange(S) + (y[k] - S // 2), np.arange(S) + (x[k] - S // 2)
        my, mx = (ys >= 0) & (ys < N), (xs >= 0) & (xs < N)
        out[k] = (kern[np.ix_(my, mx)] * F[np.ix_(ys[my], xs[mx])]).sum()
    return out


def np_imgfn(kind, kv=None, ko=None, aw=None):
    """the ImagingFunction oracle/gridref_np.do_imaging calls: (theta, lam, u, v, w, vis) -> N x N complex grid"""
    def simple(theta, lam, u, v, w, vis):
        N = P.haskell_round(theta * lam)
        return P.grid(np.zeros((N, N), dtype=np.complex128), u / np.float64(lam), v / np.float64(lam), vis)

    def conv(theta, lam, u, v, w, vis):
        N = P.haskell_round(theta * lam)
        return P.convgrid(kv, np.zeros((N, N), dtype=np.complex128), u / np.float64(lam), v / np.float64(lam), vis)

    def w_cache(theta, lam, u, v, w, vis):
        return P.w_cache_imaging(theta, lam, u, v, w, vis, ko["wstep"], ko["qpx"], ko["npixFF"], ko["npixKern"])[0]

    def aw_imaging(theta, lam, u, v, w, vis):  # (a1, a2 by position: the mirror does not swap them)
        wk, wv, ak, a1, a2 = aw
        N, S = P.haskell_round(theta * lam), wk.shape[-1]
        x, xf, y, yf = P.frac_coords((N, N), wk.shape[1], u / np.float64(lam), v / np.float64(lam))
        G = np.zeros((N, N), dtype=np.complex128)
        cache = {}
        for k in range(len(u)):
            if not (0 <= a1[k] < len(ak) and 0 <= a2[k] < len(ak)):
                continue
            kern = np.conj(aw_kernel(cache, wk, wv, ak, w[k], a1[k], a2[k], yf[k], xf[k]))
            ys, xs = np.arange(S) + (y[k] - S // 2), np.arange(S) + (x[k] - S // 2)
            my, mx = (ys >= 0) & (ys < N), (xs >= 0) & (xs < N)
            G[np.ix_(ys[my], xs[mx])] += vis[k] * kern[np.ix_(my, mx)]
        return G

    return {"simple": simple, "conv": conv, "w_cache": w_cache, "aw": aw_imaging}[kind]


def numpy_side(kind, theta, lam, uvw, vis, model, kv, aw):
    """(image of the residual, image of vis, psf, pmax, pred, residual) in numpy.  A NaN coordinate is dropped by every
    step (no weight cell, no grid cell, a zero prediction): it is moved far off the grid, where the same happens."""
    u, v, w = (x.copy() for x in uvw)
    pred = restate(kind, theta, lam, model, u, v, w, kv=kv, ko=KO, aw=aw)
    bad = np.isnan(u) | np.isnan(v)
    u[bad], v[bad] = 1e9 * lam, 1e9 * lam
    fn = np_imgfn(kind, kv=kv, ko=KO, aw=aw)
    res = vis - pred
    img, psf, pmax = P.do_imaging(theta, lam, u, v, w, res, fn)
    img0, _, _ = P.do_imaging(theta, lam, u, v, w, vis, fn)
    return img, img0, psf, pmax, pred, res


class Case:
    """one stream on the device, its imager, and the two calls the imager replaces"""

    def __init__(self, ctx, kind, theta, lam, n, seed, **kw):
        self.ctx, self.kind, self.theta, self.lam = ctx, kind, theta, lam
        self.N, self.uvw, self.vis, self.model, self.kv, self.aw = setup(kind, theta, lam, n, seed, **kw)
        self.bind()

    def bind(self, ko=KO):
        self.duvw = tuple(to_dev(x) for x in self.uvw)
        self.dvis, self.dmodel = to_dev(self.vis), to_dev(self.model)
        aw = None if self.aw is None else tuple(to_dev(x) for x in self.aw)
        self.imgfn = imgfn_of(self.kind, None if self.kv is None else to_dev(self.kv), aw, ko)
        self.a1, self.a2 = (aw[3], aw[4]) if aw is not None else (None, None)
        self.im = self.ctx.imager(self.theta, self.lam, self.duvw, self.imgfn, a1=self.a1, a2=self.a2)

    def predict(self, vis_sub=None):
        return self.ctx.predict(self.theta, self.lam, self.duvw, self.dmodel, self.imgfn, a1=self.a1, a2=self.a2,
                                vis_sub=vis_sub)

    def do_imaging(self, vis):
        return self.ctx.do_imaging(self.theta, self.lam, self.duvw, self.a1, self.a2, None, None, vis, self.imgfn)

    def cycle(self, *a, **kw):
        out = self.im.cycle(*a, **kw)
        assert self.ctx.get_option("errors") == 0
        if self.kind == "aw":
            assert self.ctx.get_option("aw_tables_built") == 0  # 6. nothing rebuilt
        return out


def against_the_calls(c):
    """item 1's comparison; returns the figures"""
    import torch
    res_ref = c.predict(vis_sub=c.dvis)
    pred_ref = c.predict()
    img_ref, psf_ref, pmax_ref = c.do_imaging(res_ref)
    img0_ref, _, _ = c.do_imaging(c.dvis)
    vis_res = torch.full_like(c.dvis, 7.0)
    img = c.cycle(c.dvis, c.dmodel, vis_res=vis_res)
    img0 = c.cycle(c.dvis)
    buf = c.dvis.clone()
    img_inplace = c.cycle(buf, c.dmodel, vis_res=buf)
    same = torch.full_like(c.dvis, 7.0)
    c.cycle(c.dvis, vis_res=same)  # without a model vis_res receives vis
    torch.cuda.synchronize()
    assert np.abs(host(img_ref)).max() > 0 and np.abs(host(pred_ref)).max() > 0
    figs = {
        "image": rel(host(img), host(img_ref)), "image, no model": rel(host(img0), host(img0_ref)),
        "image, in place": rel(host(img_inplace), host(img_ref)),
        "psf": rel(host(c.im.psf), host(psf_ref)), "pmax": abs(c.im.pmax - pmax_ref) / abs(pmax_ref),
        "predict": rel(host(c.im.predict(c.dmodel)), host(pred_ref)),
        "residual form": rel(host(c.im.predict(c.dmodel, vis_sub=c.dvis)), host(res_ref)),
        "vis_res": rel(host(vis_res), host(res_ref)), "vis_res, in place": rel(host(buf), host(res_ref)),
    }
    print(c.kind, c.N, figs)
    assert np.array_equal(host(same), c.vis)
    assert figs.pop("pmax") < 1e-12, figs
    assert max(figs.values()) < 1e-10, figs
    return pred_ref


# 1. against the calls it replaces, on the same device
@pytest.mark.parametrize("theta,lam", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_calls_it_replaces(ctx, kind, theta, lam):
    c = Case(ctx, kind, theta, lam, 3000, 11, nans=kind == "simple")
    pred = host(against_the_calls(c))
    if kind == "simple":  # NaN coordinates and cells off the grid predict exactly 0
        got = host(c.im.predict(c.dmodel))
        assert got[3] == 0 and got[5] == 0 and np.array_equal(got == 0, pred == 0) and (pred == 0).sum() > 10
    if kind == "aw":  # dropped baselines predict exactly 0 and keep their visibility in the residual
        got = host(c.im.predict(c.dmodel, vis_sub=c.dvis))
        assert all(got[k] == c.vis[k] for k in (2, 11, 17))
    c.im.close()


# 2. against numpy
@pytest.mark.parametrize("theta,lam", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_against_numpy(ctx, kind, theta, lam):
    import torch
    c = Case(ctx, kind, theta, lam, 4000, 29, nans=kind == "simple")
    img_ref, img0_ref, psf_ref, pmax_ref, pred_ref, res_ref = numpy_side(kind, theta, lam, c.uvw, c.vis, c.model, c.kv,
                                                                        c.aw)
    vis_res = torch.empty_like(c.dvis)
    img = c.cycle(c.dvis, c.dmodel, vis_res=vis_res)
    img0 = c.cycle(c.dvis)
    figs = {"image": rel(host(img), img_ref), "image, no model": rel(host(img0), img0_ref),
            "psf": rel(host(c.im.psf), psf_ref), "pmax": abs(c.im.pmax - pmax_ref) / abs(pmax_ref),
            "predict": rel(host(c.im.predict(c.dmodel)), pred_ref), "vis_res": rel(host(vis_res), res_ref)}
    print(kind, c.N, figs)
    assert np.abs(img_ref).max() > 0 and np.abs(pred_ref).max() > 0 and pmax_ref > 0
    assert max(figs.values()) < 1e-10, figs
    c.im.close()


# 3. linearity: cycle(vis, model) == cycle(vis) - cycle(predict(model))
@pytest.mark.parametrize("theta,lam", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_linearity(ctx, kind, theta, lam):
    c = Case(ctx, kind, theta, lam, 2500, 37)
    full = host(c.cycle(c.dvis, c.dmodel))
    a = host(c.cycle(c.dvis))
    b = host(c.cycle(c.im.predict(c.dmodel)))
    scale = max(np.abs(full).max(), np.abs(a).max(), np.abs(b).max())
    err = np.abs(full - (a - b)).max() / scale
    print(kind, c.N, err)
    assert scale > 0 and err < 1e-10, (kind, err)
    c.im.close()


# 4. isolation: nothing else on the context changes an imager's results, nor does overwriting its creation inputs
def test_isolation(ctx):
    import torch
    theta, lam = SHAPES[0]
    a = Case(ctx, "w_cache", theta, lam, 3000, 43)
    for t in a.duvw:  # the creation inputs, overwritten right after creation
        t.normal_().mul_(1e6)
    torch.cuda.synchronize()
    first = host(a.cycle(a.dvis, a.dmodel))
    first_psf, first_pmax = host(a.im.psf).copy(), a.im.pmax
    # another shape and w range through do_imaging (rebuilds the context's w-kernel cache), a convgrid2, an aw imager
    theta2, lam2 = SHAPES[1]
    u, v, w, vis = stream(2000, lam2, 300.0, 44)
    ko2 = {"wstep": 60, "qpx": 2, "npixFF": 16, "npixKern": 9}
    ctx.do_imaging(theta2, lam2, (to_dev(u), to_dev(v), to_dev(w)), None, None, None, None, to_dev(vis), ("w_cache", ko2))
    rng = np.random.default_rng(45)
    gcf = to_dev(rng.normal(size=(3, 2, 2, 7, 7)) + 1j * rng.normal(size=(3, 2, 2, 7, 7)))
    G = torch.zeros((96, 96), dtype=torch.complex128, device="cuda:0")
    ctx.convgrid2(gcf, G, (to_dev(u / lam2), to_dev(v / lam2), None), to_dev(rng.integers(0, 3, 2000)), to_dev(vis))
    b = Case(ctx, "aw", theta2, lam2, 1500, 46)
    b.cycle(b.dvis, b.dmodel)
    again = host(a.cycle(a.dvis, a.dmodel))
    torch.cuda.synchronize()
    assert np.abs(first).max() > 0
    assert rel(again, first) < 1e-12, rel(again, first)
    assert np.array_equal(host(a.im.psf), first_psf) and a.im.pmax == first_pmax
    a.im.close()
    b.im.close()


# 5. driver size: N = 2400 with 1.2 x 10^5 visibilities
@pytest.mark.parametrize("kind", ["w_cache", "aw"])
def test_driver_size(ctx, kind):
    theta, lam, n = 0.008, 300_000, 120_000
    c = Case.__new__(Case)
    c.ctx, c.kind, c.theta, c.lam, c.N = ctx, kind, theta, lam, P.haskell_round(theta * lam)
    assert c.N == 2400
    rng = np.random.default_rng(77)
    c.uvw = (rng.uniform(-0.45, 0.45, n) * lam, rng.uniform(-0.45, 0.45, n) * lam, rng.uniform(-1800.0, 1800.0, n))
    c.vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    c.model = rng.normal(size=(c.N, c.N))
    c.kv, c.aw = None, None
    if kind == "aw":
        c.aw = aw_tables(5, 4, 15, 8, 1800.0, 78) + (rng.integers(0, 8, n), rng.integers(0, 8, n))
    c.bind(ko={"wstep": 500, "qpx": 4, "npixFF": 64, "npixKern": 15})
    against_the_calls(c)
    c.im.close()


def test_aw_stream_of_several_batches(ctx):
    """above the aw batch size (2^20) on a small grid: the imager holds two batches per record set"""
    theta, lam = SHAPES[0]
    n = (1 << 20) + 5000
    c = Case.__new__(Case)
    c.ctx, c.kind, c.theta, c.lam = ctx, "aw", theta, lam
    c.N, c.uvw, c.vis, c.model, c.kv, c.aw = setup("aw", theta, lam, n, 51)
    c.bind()
    assert ctx.get_option("aw_tables_built") == 4  # two batches, two streams
    against_the_calls(c)
    c.im.close()


# 7. a cycle can be captured into a graph and replayed
def test_cycle_can_be_captured_into_a_hip_graph(ctx):
    """After a warm-up cycle on the capture stream a cycle enqueues nothing but kernel launches (the tile kernels, the
    imager's own, hipFFT's): no allocation, no synchronisation, no read-back, no memset node.  Three replays with changed
    model contents must reproduce the eager result."""
    import torch
    theta, lam = SHAPES[0]
    N = P.haskell_round(theta * lam)
    u, v, w, vis = stream(20000, lam, 100.0, 61, span=0.3)  # every baseline inside the grid
    rng = np.random.default_rng(62)
    duvw, dvis = tuple(to_dev(x) for x in (u, v, w)), to_dev(vis)
    dmodel = to_dev(rng.normal(size=(N, N)))
    im = ctx.imager(theta, lam, duvw, ("w_cache", KO))
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        im.cycle(dvis, dmodel, out=img)  # warm-up on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        im.cycle(dvis, dmodel, out=img)
    torch.cuda.synchronize()
    errs = []
    for i in range(3):
        dmodel.copy_(to_dev(rng.normal(size=(N, N)) * (i + 1)))
        img.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = host(img).copy()
        eager = host(im.cycle(dvis, dmodel))
        errs.append(rel(got, eager))
    errors = ctx.get_option("errors")
    print(errs)
    assert np.abs(eager).max() > 0 and max(errs) < 1e-12 and errors == 0, errs
    im.close()


# 8. refusals and edges
def test_empty_imager(ctx):
    import torch
    theta, lam = SHAPES[0]
    e = torch.empty(0, dtype=torch.float64, device="cuda:0")
    for imgfn, a in ((("simple",), None), (("w_cache", KO), None),
                     (("aw",) + tuple(to_dev(x) for x in aw_tables(3, 2, 9, A, 100.0, 1)),
                      torch.empty(0, dtype=torch.int64, device="cuda:0"))):
        im = ctx.imager(theta, lam, (e, e, e), imgfn, a1=a, a2=a)
        img = torch.full((64, 64), 3.0, dtype=torch.float64, device="cuda:0")
        im.cycle(torch.empty(0, dtype=torch.complex128, device="cuda:0"), out=img)
        assert torch.count_nonzero(img).item() == 0 and torch.count_nonzero(im.psf).item() == 0
        im.close()


def test_refusals(ctx):
    import torch
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    theta, lam = SHAPES[0]
    c = Case(ctx, "conv", theta, lam, 500, 71)
    q = lambda t: C.c_void_p(t.data_ptr())
    img = torch.full((c.N, c.N), 3.0, dtype=torch.float64, device="cuda:0")
    out = torch.full_like(c.dvis, 5.0)
    assert lib.gridhip_imager_cycle_dev(c.im._h, q(c.dmodel), None, q(img), q(out)) == _lib.EINVAL
    assert lib.gridhip_imager_cycle_dev(c.im._h, q(c.dmodel), q(c.dvis), None, q(out)) == _lib.EINVAL
    assert lib.gridhip_imager_predict_dev(c.im._h, None, None, q(out)) == _lib.EINVAL
    assert lib.gridhip_imager_predict_dev(c.im._h, q(c.dmodel), None, None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.all(img == 3.0).item() and torch.all(out == 5.0).item()
    c.im.close()
    c.im.close()  # (closing twice is harmless)
    u, v, w = c.duvw
    kv = c.imgfn[1]
    ih = C.c_void_p(0x1234)
    create = lambda *a: lib.gridhip_imager_create_dev(h, *a, C.byref(ih))
    assert create(9, 0, 0, 0, 0, 0, None, theta, lam, 500, q(u), q(v), q(w), 1) == _lib.EINVAL and not ih.value
    assert create(1, 0, 4, 0, 7, 7, None, theta, lam, 500, q(u), q(v), q(w), 1) == _lib.EINVAL  # conv without kv
    assert create(1, 0, 4, 0, 7, 7, q(kv), theta, lam, 500, None, q(v), q(w), 1) == _lib.EINVAL
    assert create(2, 40, 2, 8, 9, 9, None, theta, lam, 500, q(u), q(v), q(w), 1) == _lib.EINVAL  # npixKern > npixFF
    assert create(2, 40, 2, 16, 7, 7, None, theta, lam, 500, q(u), q(v), None, 1) == _lib.EINVAL  # w_cache without w
    assert create(0, 0, 0, 0, 0, 0, None, theta, lam, 500, q(u), q(v), q(w), 0) == _lib.EINVAL  # stride
    assert lib.gridhip_imager_create_dev(h, 0, 0, 0, 0, 0, 0, None, theta, lam, 500, q(u), q(v), q(w), 1, None) == _lib.EINVAL
    # unsupported at creation: nothing is half-created
    ih = C.c_void_p(0x1234)
    wide = to_dev(np.linspace(-40000.0, 40000.0, 500))  # 80 001 planes at wstep 1
    assert create(2, 1, 2, 16, 7, 7, None, theta, lam, 500, q(u), q(v), q(wide), 1) == _lib.EUNSUPPORTED and not ih.value
    ih = C.c_void_p(0x1234)
    big = torch.zeros(64 * 64 * 4, dtype=torch.complex128, device="cuda:0")
    a1 = torch.zeros(500, dtype=torch.int64, device="cuda:0")
    wv = to_dev(np.linspace(-1.0, 1.0, 2))
    assert lib.gridhip_imager_create_aw_dev(h, theta, lam, 2, 1, 64, 1, q(big), q(wv), q(big), 500, q(u), q(v), q(w), 1,
                                            q(a1), q(a1), C.byref(ih)) == _lib.EUNSUPPORTED and not ih.value  # S > 63
    assert lib.gridhip_imager_create_aw_dev(h, theta, lam, 2, 1, 9, 0, q(big), q(wv), q(big), 500, q(u), q(v), q(w), 1,
                                            q(a1), q(a1), C.byref(ih)) == _lib.EINVAL  # A = 0
    assert lib.gridhip_imager_destroy(None) == 0
    # the context is as usable as before
    c2 = Case(ctx, "conv", theta, lam, 500, 71)
    against_the_calls(c2)
    c2.im.close()
