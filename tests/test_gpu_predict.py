"""Prediction on the GPU (gridhip_predict[_aw][_dev], Context.predict): parity per kind with a numpy restatement built
from oracle/gridref_np, the adjoint identity against the library's own imaging functions, a point source, the residual
form (also in place), host and device forms, refused calls, and a driver-sized stream for w_cache and aw."""
import ctypes as C

import numpy as np
import pytest

from oracle import gridref_np as P

pytestmark = pytest.mark.gpu

KO = {"wstep": 40, "qpx": 2, "npixFF": 16, "npixKern": 7}
SHAPES = [(0.1, 640), (0.1, 490)]  # N = 64 (even) and N = 49 (odd)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


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


# ---- numpy restatement of the prediction: pred = A^H fft_c(model) -------------------------------------------------
def restate(kind, theta, lam, model, u, v, w, kv=None, ko=None, aw=None, F=None):
    """aw = (wk, wvals, ak, a1, a2); F: fft_c(model) when already known"""
    N = model.shape[0]
    F = P.fft_c(model.astype(np.complex128)) if F is None else F
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
    W, Q, _, S, _ = wk.shape
    x, xf, y, yf = P.frac_coords((N, N), Q, pu, pv)
    out = np.zeros(len(u), dtype=np.complex128)
    cache = {}
    for k in range(len(u)):
        if not (0 <= a1[k] < len(ak) and 0 <= a2[k] < len(ak)):
            continue
        wb = P.find_closest(wv, w[k])
        key = (wb, a1[k], a2[k], yf[k], xf[k])
        if key not in cache:
            cache[key] = P.aw_kernel_fn2(yf[k], xf[k], wk[wb], ak[a1[k]], ak[a2[k]])
        ys, xs = np.arange(S) + (y[k] - S // 2), np.arange(S) + (x[k] - S // 2)
        my, mx = (ys >= 0) & (ys < N), (xs >= 0) & (xs < N)
        out[k] = (cache[key][np.ix_(my, mx)] * F[np.ix_(ys[my], xs[mx])]).sum()
    return out


def imgfn_of(kind, kv=None, aw=None):
    if kind == "simple":
        return ("simple",)
    if kind == "conv":
        return ("conv", kv)
    if kind == "w_cache":
        return ("w_cache", KO)
    return ("aw", aw[0], aw[1], aw[2])


def setup(kind, theta, lam, n, seed, nans=False):
    N = P.haskell_round(theta * lam)
    u, v, w, vis = stream(n, lam, 100.0, seed, nans=nans)
    rng = np.random.default_rng(seed + 1)
    model = rng.normal(size=(N, N))
    kv = kv_table(4, 7, seed) if kind == "conv" else None
    aw = None
    if kind == "aw":
        wk, wv, ak = aw_tables(3, 2, 9, 4, 100.0, seed)
        aw = (wk, wv, ak, rng.integers(0, 4, n), rng.integers(0, 4, n))
    return N, (u, v, w), vis, model, kv, aw


def predict(ctx, kind, theta, lam, uvw, model, kv=None, aw=None, vis_sub=None, out=None):
    a1, a2 = (aw[3], aw[4]) if aw is not None else (None, None)
    return ctx.predict(theta, lam, uvw, model, imgfn_of(kind, kv, aw), a1=a1, a2=a2, vis_sub=vis_sub, out=out)


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


KINDS = ["simple", "conv", "w_cache", "aw"]


# 1. parity per kind with the restatement, host and device forms, even and odd N
@pytest.mark.parametrize("theta,lam", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_restatement(ctx, kind, theta, lam):
    n = 400 if kind == "aw" else 3000
    N, uvw, _, model, kv, aw = setup(kind, theta, lam, n, 11, nans=kind == "simple")
    got = predict(ctx, kind, theta, lam, uvw, model, kv, aw)
    ref = restate(kind, theta, lam, model, *uvw, kv=kv, ko=KO, aw=aw)
    assert np.abs(ref).max() > 0
    assert rel(got, ref) < 1e-12, (kind, N, rel(got, ref))
    if kind == "simple":  # off the grid's edge and NaN: exactly 0
        off = (np.abs(np.floor(0.5 + N * (uvw[0] / lam))) > N // 2 - 1) | np.isnan(uvw[0]) | np.isnan(uvw[1])
        assert off.sum() > 10 and np.all(got[np.isnan(uvw[0]) | np.isnan(uvw[1])] == 0)
        assert np.all(got[ref == 0] == 0)
    dgot = predict(ctx, kind, theta, lam, tuple(to_dev(x) for x in uvw), to_dev(model),
                   None if kv is None else to_dev(kv),
                   None if aw is None else tuple(to_dev(x) for x in aw))
    assert np.array_equal(dgot.cpu().numpy(), got), kind  # 5. host and device forms are bit-identical


# 2. the adjoint identity against the library's own imaging functions
@pytest.mark.parametrize("theta,lam", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_of_the_imaging_function(ctx, kind, theta, lam):
    n = 2000
    N, uvw, vis, model, kv, aw = setup(kind, theta, lam, n, 23, nans=kind == "simple")
    if kind == "simple":
        G = ctx.simple_imaging(theta, lam, uvw, None, vis)
    elif kind == "conv":
        G = ctx.conv_imaging(kv, theta, lam, uvw, None, vis)
    elif kind == "w_cache":
        G = ctx.w_cache_imaging(KO, theta, lam, uvw, None, vis)
    else:
        G = ctx.aw_imaging(theta, lam, aw[0], aw[1], aw[2], uvw, (aw[3], aw[4]), vis)
    img = np.real(P.ifft_c(G))
    model = img / np.abs(img).max() + 0.1 * model  # (correlated with the image: lhs is far from 0)
    lhs = np.sum(model * img)
    pred = predict(ctx, kind, theta, lam, uvw, model, kv, aw)
    rhs = np.real(np.vdot(vis, pred)) / (N * N)
    assert abs(lhs - rhs) < 1e-10 * abs(lhs), (kind, N, lhs, rhs)


# 3. a unit point source at the centre pixel predicts 1 at every in-grid visibility of the simple kind
@pytest.mark.parametrize("theta,lam", SHAPES)
def test_point_source(ctx, theta, lam):
    N, uvw, _, _, _, _ = setup("simple", theta, lam, 5000, 5)
    model = np.zeros((N, N))
    model[N // 2, N // 2] = 1.0
    got = predict(ctx, "simple", theta, lam, uvw, model)
    x = N // 2 + np.floor(0.5 + N * (uvw[0] / lam))
    y = N // 2 + np.floor(0.5 + N * (uvw[1] / lam))
    inside = (x >= 0) & (y >= 0) & (x < N) & (y < N)
    assert inside.sum() > 100 and (~inside).sum() > 100
    assert np.abs(got[inside] - 1).max() < 1e-14
    assert np.all(got[~inside] == 0)


# 4. the residual form: vis_sub - predict(model), bit-identical, also in place
@pytest.mark.parametrize("kind", KINDS)
def test_residual(ctx, kind):
    theta, lam = SHAPES[1]
    N, uvw, vis, model, kv, aw = setup(kind, theta, lam, 600, 31)
    pred = predict(ctx, kind, theta, lam, uvw, model, kv, aw)
    res = predict(ctx, kind, theta, lam, uvw, model, kv, aw, vis_sub=vis)
    assert np.array_equal(res, vis - pred)
    buf = vis.copy()
    r2 = predict(ctx, kind, theta, lam, uvw, model, kv, aw, vis_sub=buf, out=buf)
    assert r2 is buf and np.array_equal(buf, vis - pred)
    dbuf = to_dev(vis)
    dres = predict(ctx, kind, theta, lam, tuple(to_dev(x) for x in uvw), to_dev(model),
                   None if kv is None else to_dev(kv), None if aw is None else tuple(to_dev(x) for x in aw),
                   vis_sub=dbuf, out=dbuf)
    assert dres is dbuf and np.array_equal(dbuf.cpu().numpy(), vis - pred)


def test_residual_keeps_dropped_visibilities_and_counts_them(ctx):
    theta, lam = SHAPES[0]
    N, uvw, vis, model, _, aw = setup("aw", theta, lam, 500, 41)
    a1, a2 = aw[3].copy(), aw[4].copy()
    a1[0], a2[7] = 4, -1  # antennas out of range
    aw = aw[:3] + (a1, a2)
    res = predict(ctx, "aw", theta, lam, uvw, model, aw=aw, vis_sub=vis)
    assert ctx.last_dropped() == 2
    assert res[0] == vis[0] and res[7] == vis[7]
    pred = predict(ctx, "aw", theta, lam, uvw, model, aw=aw)
    assert pred[0] == 0 and pred[7] == 0 and np.count_nonzero(pred) > 400
    ref = restate("aw", theta, lam, model, *uvw, aw=aw)
    assert rel(pred, ref) < 1e-12


# 5. a refused call leaves vis_out untouched
def test_refused_calls_leave_vis_out_untouched(ctx):
    theta, lam = SHAPES[0]
    N, uvw, _, model, _, _ = setup("simple", theta, lam, 100, 3)
    u, v, w = (np.ascontiguousarray(x) for x in uvw)
    p = lambda a: C.c_void_p(a.ctypes.data)
    lib = ctx._lib
    out = np.full(100, 3 - 4j)
    for kind in (9, -1):
        assert lib.gridhip_predict(ctx._h, kind, 0, 0, 0, 0, 0, None, theta, lam, p(model), 100, p(u), p(v), p(w), 1,
                                   None, p(out)) == -1
    assert lib.gridhip_predict(ctx._h, 1, 0, 4, 0, 7, 7, None, theta, lam, p(model), 100, p(u), p(v), p(w), 1, None,
                               p(out)) == -1  # conv without kv
    assert lib.gridhip_predict(ctx._h, 0, 0, 0, 0, 0, 0, None, theta, lam, None, 100, p(u), p(v), p(w), 1, None,
                               p(out)) == -1
    assert lib.gridhip_predict(ctx._h, 2, 40, 2, 8, 9, 9, None, theta, lam, p(model), 100, p(u), p(v), p(w), 1, None,
                               p(out)) == -1  # npixKern > npixFF
    assert np.all(out == 3 - 4j)
    dout = to_dev(out)
    du, dv, dw, dm = to_dev(u), to_dev(v), to_dev(w), to_dev(model)
    q = lambda t: C.c_void_p(t.data_ptr())
    assert lib.gridhip_predict_dev(ctx._h, 5, 0, 0, 0, 0, 0, None, theta, lam, q(dm), 100, q(du), q(dv), q(dw), 1, None,
                                   q(dout)) == -1
    assert lib.gridhip_predict_aw_dev(ctx._h, theta, lam, 3, 2, 9, 0, q(dm), q(dm), q(dm), q(dm), 100, q(du), q(dv),
                                      q(dw), 1, q(du), q(du), None, q(dout)) == -1  # A = 0
    ctx.synchronize()
    assert np.all(dout.cpu().numpy() == 3 - 4j)
    with pytest.raises(ValueError):
        ctx.predict(theta, lam, uvw, model[:-1], ("simple",))


# 6. driver size: N = 2400, 10^6 visibilities, checked on a sample of 10^4
@pytest.mark.parametrize("kind", ["w_cache", "aw"])
def test_driver_size(ctx, kind):
    import torch
    theta, lam, n = 0.08, 30000, 1_000_000
    N = P.haskell_round(theta * lam)
    assert N == 2400
    rng = np.random.default_rng(77)
    u = rng.uniform(-0.45, 0.45, n) * lam
    v = rng.uniform(-0.45, 0.45, n) * lam
    w = rng.uniform(-1800.0, 1800.0, n)
    model = rng.normal(size=(N, N))
    ko = {"wstep": 500, "qpx": 4, "npixFF": 64, "npixKern": 15}
    if kind == "w_cache":
        imgfn, aw = ("w_cache", ko), None
        a1 = a2 = None
    else:
        wk, wv, ak = aw_tables(5, 4, 15, 8, 1800.0, 78)
        a1, a2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
        imgfn, aw = ("aw", to_dev(wk), to_dev(wv), to_dev(ak)), (wk, wv, ak)
    got = ctx.predict(theta, lam, (to_dev(u), to_dev(v), to_dev(w)), to_dev(model), imgfn,
                      a1=None if a1 is None else to_dev(a1), a2=None if a2 is None else to_dev(a2))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert np.count_nonzero(got) > 0.99 * n
    F = P.fft_c(model.astype(np.complex128))
    s = rng.choice(n, 10_000, replace=False)
    if kind == "w_cache":
        # the planes of the whole stream (the w-bin rule takes its min and max), gathered for the sample only
        wb, wmin, steps = P.wbins(w, ko["wstep"])
        kerns = np.stack([P.w_kernel(theta, float(i * ko["wstep"] + wmin), ko["npixFF"], ko["npixKern"], ko["qpx"])
                          for i in range(steps)])
        ref = P.degrid2(kerns, F, u[s] / np.float64(lam), v[s] / np.float64(lam), wb[s])
    else:
        ref = restate("aw", theta, lam, model, u[s], v[s], w[s], aw=aw + (a1[s], a2[s]), F=F)
    assert rel(got[s], ref) < 1e-12, rel(got[s], ref)
