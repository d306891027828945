"""Image-domain layers of the w-stack (include/gridhip.h, "w-stacking", IMAGE-DOMAIN LAYERS), the checks that need no GPU:
the numpy restatement the GPU tests compare with (tests/idg_ref.py) is two to seven orders of magnitude closer to a direct
Fourier sum than the stacked w-projection of tests/wstack_ref.py on that file's own cases; its predict is the exact adjoint
of its image, clipped subgrids, dropped visibilities and a NaN w included; the tile arithmetic and the trusted-region rule
on hand-computed cases; and the binding hands ("idg", ...) to the w-stacking symbols with qpx = 0 and refuses bad options
before any call (against the recording library of test_binding_marshalling.py)."""
import ctypes as C

import numpy as np
import pytest

import idg_ref as I
import wstack_ref as W
from test_binding_marshalling import HANDLE, Arr, Out, Ref
from test_weights_host import SameT, rig, torch_rig  # noqa: F401  (fixtures)
from test_wstack_host import CASES

f64, c128 = np.float64, np.complex128


# ---- 1: accuracy against a direct Fourier sum -----------------------------------------------------------------------------------
def fourier_case(case):
    """test_wstack_host.py's stream of the case and its direct sum"""
    theta, lam, wstep, M, S, ff, q, wmax = case
    rng = np.random.default_rng(1)
    n = 300
    u = rng.uniform(-0.35 * lam, 0.35 * lam, n)
    v = rng.uniform(-0.35 * lam, 0.35 * lam, n)
    w = rng.uniform(-wmax, wmax, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    N = W.image_size(theta, lam)
    c = (np.arange(N) - N // 2) / N * theta
    cx, cy = c[None, :], c[:, None]
    ph = 1.0 - np.sqrt(1.0 - cx * cx - cy * cy)
    direct = np.zeros((N, N), dtype=c128)
    for k in range(n):
        direct += vis[k] * np.exp(2j * np.pi * (u[k] * cx + v[k] * cy - w[k] * ph))
    direct /= N * N
    return N, u, v, w, vis, direct


@pytest.mark.parametrize("case", CASES, ids=["N64-M5", "N64-M4-wide", "N65-M3"])
def test_image_domain_layers_against_a_direct_fourier_sum(case):
    """err(A) = max|A - I| / max|I|, I the direct sum, over the inner half as test_wstack_host.py takes it and over the
    trusted region.  Measured with the restatement: inner half (16, 8) 3.5e-4 / 1.5e-3 / 1.5e-4, (24, 12) 3.1e-6 / 2.9e-5 /
    1.5e-6, (32, 16) 4.9e-8 / 6.4e-7 / 2.5e-8; trusted region (24, 12) 5.4e-5 / 5.1e-4 / 3.1e-5; the stacked w-projection
    0.203 / 0.169 / 0.199."""
    theta, lam, wstep, M, S, ff, q, wmax = case
    N, u, v, w, vis, direct = fourier_case(case)
    inner, tr = slice(N // 4, N - N // 4), I.trusted(N)

    def err(A, s):
        return np.abs(A[s, s] - direct[s, s]).max() / np.abs(direct[s, s]).max()

    stacked = err(W.Stack(theta, lam, u, v, w, wstep, M, q, ff, S).dirty(vis), inner)
    got = {sk: I.Stack(theta, lam, u, v, w, wstep, M, *sk).dirty(vis) for sk in ((16, 8), (24, 12), (32, 16))}
    e16, e32, e24t = err(got[16, 8], inner), err(got[32, 16], inner), err(got[24, 12], tr)
    print(f"N={N} M={M}: stacked w-projection {stacked:.4f}; inner half (16, 8) {e16:.3e} (ratio {e16 / stacked:.4f}) "
          f"(24, 12) {err(got[24, 12], inner):.3e} (32, 16) {e32:.3e}; trusted region (24, 12) {e24t:.3e}")
    assert e16 <= 0.02 * stacked
    assert e32 <= 1e-5
    assert e24t <= 5e-3
    for A in got.values():  # outside the trusted region the image is exactly 0
        out = np.ones((N, N), dtype=bool)
        out[tr, tr] = False
        assert not A[out].any() and A[tr, tr].all()


# ---- 2: the adjoint identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [640, 650], ids=["N64", "N65"])
@pytest.mark.parametrize("sk", [(16, 4), (24, 12), (32, 16)], ids=str)
def test_restatement_predict_is_the_adjoint_of_image(lam, sk):
    theta, n = 0.1, 300
    rng = np.random.default_rng(11)
    N = W.image_size(theta, lam)
    u, v = rng.uniform(-0.52 * lam, 0.52 * lam, n), rng.uniform(-0.52 * lam, 0.52 * lam, n)
    w = rng.uniform(-1500, 1500, n)
    w[5] = np.nan
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))  # (the whole plane: predict reads the trusted region only, through C)
    st = I.Stack(theta, lam, u, v, w, 100, 4, *sk)
    assert 1 < st.dropped < n // 4 and not st.keep[5]
    assert min(st.ox[st.keep].min(), st.oy[st.keep].min()) < 0
    assert max(st.ox[st.keep].max(), st.oy[st.keep].max()) + sk[0] > N  # subgrids clipped on either side
    pred = st.predict(model)
    lhs = np.sum(model * st.image(vis))
    rhs = np.real(np.vdot(vis, pred)) / (N * N)
    print(f"N={N} {sk}: adjoint identity to {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e}")
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    assert not pred[~st.keep].any() and pred[st.keep].all()
    assert np.array_equal(st.predict(model, vis_sub=vis)[~st.keep], vis[~st.keep])


# ---- 3: tiles, subgrids and the trusted region on hand-computed cases -----------------------------------------------------------------
def test_tile_arithmetic():
    eps = 2.0 ** -40
    # N = 64, (16, 8): T = 8, origins -4, 4, 12 ..., centres 4, 12, 20 ...
    keep, t, o, a = I.tiles(np.array([0.0, 7.5, 8.0, 8.0 - eps, 64 - eps, 64.0, -eps, np.nan, 63.0]), 64, 16, 8)
    assert np.array_equal(keep, [True, True, True, True, True, False, False, False, True])
    assert np.array_equal(t[keep], [0, 0, 1, 0, 7, 7]) and np.array_equal(o[keep], [-4, -4, 4, -4, 52, 52])
    assert np.array_equal(a[keep], [-4.0, 3.5, -4.0, 4.0 - eps, 4.0 - eps, 3.0])  # on a boundary: the upper tile, a = -T / 2
    assert not t[~keep].any() and not a[~keep].any()
    # odd N, T = 12 does not divide it: N = 65, (16, 4); the last tile 5 starts at 60 and its subgrid ends at 74 > N
    keep, t, o, a = I.tiles(np.array([59.999, 60.0, 64.99, 65.0, 32.0]), 65, 16, 4)
    assert np.array_equal(keep, [True, True, True, False, True])
    assert np.array_equal(t[keep], [4, 5, 5, 2]) and np.array_equal(o[keep], [46, 58, 58, 22])
    assert np.allclose(a[keep], [59.999 - 54, -6.0, 64.99 - 66, 2.0], rtol=0, atol=1e-13) and a[1] == -6.0
    # (24, 12) and (32, 16): T = 12, 16
    keep, t, o, a = I.tiles(np.array([12.0, 11.0]), 64, 24, 12)
    assert np.array_equal(t, [1, 0]) and np.array_equal(o, [6, -6]) and np.array_equal(a, [-6.0, 5.0])
    keep, t, o, a = I.tiles(np.array([16.0, 47.25]), 64, 32, 16)
    assert np.array_equal(t, [1, 2]) and np.array_equal(o, [8, 24]) and np.array_equal(a, [-8.0, 7.25])
    # the stack's cell coordinate: x = N (u / lam) + N div 2
    st = I.Stack(0.1, 650, np.array([0.0, 325.0, -320.0, -330.0]), np.zeros(4), np.zeros(4), 100, 1, 16, 4)
    assert st.N == 65 and np.array_equal(st.keep, [True, True, True, False]) and st.dropped == 1
    assert np.array_equal(st.tx[st.keep], [2, 5, 0]) and np.array_equal(st.a[st.keep], [2.0, -1.5, -6.0])


def test_trusted_region_rule():
    # 8 |x - N div 2| <= 3 N: N = 64 -> |d| <= 24 (equality at 8 and 56: inside); N = 65 -> |d| <= 24.375; N = 16 -> |d| <= 6
    for N, lo, hi in ((64, 8, 56), (65, 8, 56), (16, 2, 14), (2048, 256, 1792)):
        c = I.correction1(N, 8)
        assert np.array_equal(np.flatnonzero(c), np.arange(lo, hi + 1)) and I.trusted(N) == slice(lo, hi + 1)
    c = I.correction1(64, 16)
    assert c[32] == 1.0 and c[7] == 0.0 and c[57] == 0.0
    assert c[8] == pytest.approx(np.exp(1.15 * 16 * (1.0 - np.sqrt(1.0 - 4.0 * (24 / 64) ** 2)))) and c[8] == c[56]
    assert 2.5e5 < c[8] ** 2 < 2.7e5  # (the 2.6e5 of the corner at (32, 16))
    import gridhip
    for N in (16, 64, 65, 100, 2048):
        assert gridhip.idg_trusted(N) == I.trusted(N)
    with pytest.raises(ValueError):
        I.check(20, 8)


# ---- 4: marshalling -----------------------------------------------------------------------------------------------------------------
THETA, LAM, NPIX, NV = 0.008, 2000, 16, 6
OPTS = dict(wstep=40, planes=3, subgrid=16, margin=6)
SPEC = [40, 3, 0, 6, 16, THETA, LAM]


def stream():
    u = (np.arange(NV, dtype=np.float32) - 2) * 8
    v = (np.arange(2 * NV, dtype=f64))[::2]
    w = [float(k) * 30 - 70 for k in range(NV)]
    vis = (np.arange(NV) - 1j * (np.arange(NV) % 3)).astype(np.complex64)
    return u, v, w, vis


def test_options_map_to_qpx_0():
    from gridhip._marshal import HOST, idg_options, imaging_function, stack_options
    assert idg_options(OPTS) == (40, 3, 0, 6, 16)
    assert idg_options(dict(planes=2, subgrid=32, margin=16)) == (2000, 2, 0, 16, 32)
    assert idg_options(dict(wstep=0, planes=2, subgrid=24, margin=4)) == (2000, 2, 0, 4, 24)
    assert imaging_function(HOST, ("idg", OPTS)) == (4, 40, 0, 6, 16, 3, None)
    assert stack_options(("idg", OPTS)) == (40, 3, 0, 6, 16)
    assert stack_options(("wstack", dict(wstep=40, planes=3, qpx=2, npixFF=8, npixKern=5))) == (40, 3, 2, 8, 5)
    with pytest.raises(ValueError):
        stack_options(("w_cache", OPTS))


def test_host_forms_reach_the_stack(rig):
    ctx, rec, run = rig
    u, v, w, vis = stream()
    img, psf = Out(f64, NPIX * NPIX), Out(f64, NPIX * NPIX)
    got = run(lambda: ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("idg", OPTS)),
              "gridhip_do_imaging_wstack", *SPEC, NV, Arr(u, f64), Arr(v, f64), Arr(w, f64), 1, Arr(vis, c128), img, psf,
              Ref(C.c_double, 2.5))
    assert img.returned(got[0], (NPIX, NPIX)) and psf.returned(got[1], (NPIX, NPIX)) and got[2] == 2.5
    model = np.arange(NPIX * NPIX, dtype=np.float32).reshape(NPIX, NPIX)
    o = Out(c128, NV)
    got = run(lambda: ctx.predict(THETA, LAM, (u, v, w), model, ("idg", OPTS)), "gridhip_predict_wstack", *SPEC,
              Arr(model, f64), NV, Arr(u, f64), Arr(v, f64), Arr(w, f64), 1, None, o)
    assert o.returned(got, (NV,))


class Anything:
    def check(self, arg, where):
        assert arg is not None, where


def test_device_forms_and_handles_reach_the_stack(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    u, v, w = (torch.arange(NV, dtype=torch.float64) * 3 + k for k in range(3))
    vis = torch.ones(NV, dtype=torch.complex128)
    model = torch.ones((NPIX, NPIX), dtype=torch.float64)
    uvw = [NV, SameT(u), SameT(v), SameT(w), 1]
    run(lambda: ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("idg", OPTS)),
        "gridhip_do_imaging_wstack_dev", *SPEC, *uvw, SameT(vis), Anything(), Anything(), Ref(C.c_double, 1.5))
    out = run(lambda: ctx.predict(THETA, LAM, (u, v, w), model, ("idg", OPTS), vis_sub=vis, out=vis),
              "gridhip_predict_wstack_dev", *SPEC, SameT(model), *uvw, SameT(vis), SameT(vis))
    assert out is vis
    hp = Ref(C.c_void_p, 0xABCD)
    ws = run(lambda: ctx.wstack(THETA, LAM, (u, v, w), ("idg", OPTS)), "gridhip_wstack_create_dev", *SPEC, *uvw, hp)
    assert ws.n == NV and ws.N == NPIX
    ws._h = None
    head = [4, 40, 0, 6, 16, 3, None, THETA, LAM, *uvw]
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("idg", OPTS)), "gridhip_imager_create_dev", *head, hp)
    made._h = None
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("idg", OPTS), weighting="natural"),
               "gridhip_imager_create_weighted_dev", *head, 0, 0.0, 0.0, None, hp)
    made._h = None
    # the w-projection stack goes the way it went, as a dict and as a tuple
    ko = dict(wstep=40, planes=3, qpx=2, npixFF=8, npixKern=5)
    for arg in (ko, ("wstack", ko)):
        ws = run(lambda: ctx.wstack(THETA, LAM, (u, v, w), arg), "gridhip_wstack_create_dev", 40, 3, 2, 8, 5, THETA, LAM, *uvw, hp)
        ws._h = None


@pytest.mark.parametrize("bad", [dict(subgrid=20), dict(margin=5), dict(margin=2), dict(margin=10), dict(planes=0),
                                 dict(subgrid=32, margin=18), dict(wstep=-1)], ids=str)
def test_bad_options_raise_before_any_call(torch_rig, bad):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    u, v, w, vis = stream()
    opts = dict(OPTS, **bad)
    model = np.zeros((NPIX, NPIX))
    t = tuple(torch.zeros(NV, dtype=torch.float64) for _ in range(3))
    with pytest.raises(ValueError, match="idg:"):
        ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("idg", opts))
    with pytest.raises(ValueError, match="idg:"):
        ctx.predict(THETA, LAM, (u, v, w), model, ("idg", opts))
    with pytest.raises(ValueError, match="idg:"):
        ctx.wstack(THETA, LAM, t, ("idg", opts))
    with pytest.raises(ValueError, match="idg:"):
        ctx.imager(THETA, LAM, t, ("idg", opts))
    assert rec.calls == []


def test_the_w_projection_stack_still_refuses_qpx_0(rig):
    ctx, rec, run = rig
    u, v, w, vis = stream()
    ko = dict(wstep=40, planes=3, qpx=0, npixFF=8, npixKern=16)
    with pytest.raises(ValueError, match="wstack:"):
        ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("wstack", ko))
    with pytest.raises(ValueError, match="wstack:"):
        ctx.wstack(THETA, LAM, (u, v, w), ko)
    with pytest.raises(KeyError):
        ctx.predict(THETA, LAM, (u, v, w), np.zeros((NPIX, NPIX)), ("idg", dict(planes=3, subgrid=16)))
    assert rec.calls == []


def test_a_null_context_is_refused_and_nothing_is_touched():
    from gridhip import _lib
    lib = _lib.load()
    x = np.zeros(64)
    p = C.c_void_p(x.ctypes.data)
    h = C.c_void_p(0x1234)
    assert lib.gridhip_wstack_create_dev(None, 100, 2, 0, 8, 16, 0.1, 160, 4, p, p, p, 1, C.byref(h)) == _lib.EINVAL
    assert h.value == 0x1234
    pm = C.c_double(7.0)
    for fn in (lib.gridhip_do_imaging_wstack, lib.gridhip_do_imaging_wstack_dev):
        assert fn(None, 100, 2, 0, 8, 16, 0.1, 160, 4, p, p, p, 1, p, p, p, C.byref(pm)) == _lib.EINVAL
    assert pm.value == 7.0 and not x.any()
