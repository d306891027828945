"""W-stacking (include/gridhip.h, "w-stacking"), the checks that need no GPU: the numpy restatement the GPU tests compare
with (tests/wstack_ref.py) has the screen's sign right and is more accurate than un-stacked w-projection at equal support,
against a direct Fourier sum; its predict is the exact adjoint of its image; M = 1 degenerates as it must; the layer
arithmetic on hand-computed cases; and Context.do_imaging / Context.predict hand ("wstack", ...) to the new symbols
(against the recording library of test_binding_marshalling.py) and refuse bad options before any call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wstack_ref as W
from conftest import ROOT
from oracle import gridref_np as R
from test_binding_marshalling import HANDLE, Arr, Out, Ref

f64, c128, i64 = np.float64, np.complex128, np.int64

NAMES = ["gridhip_wstack_create_dev", "gridhip_wstack_image_dev", "gridhip_wstack_predict_dev", "gridhip_wstack_info",
         "gridhip_wstack_destroy", "gridhip_do_imaging_wstack", "gridhip_do_imaging_wstack_dev", "gridhip_predict_wstack",
         "gridhip_predict_wstack_dev"]

# (theta, lam, wstep, M, S, npixFF, qpx, wmax)
CASES = [(0.1, 640, 100, 5, 9, 32, 2, 2000), (0.2, 320, 50, 4, 7, 24, 4, 1500), (0.1, 650, 100, 3, 9, 32, 2, 2000)]


# ---- 1: the sign and the benefit, against a direct Fourier sum ---------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=["N64-M5", "N64-M4-wide", "N65-M3"])
def test_stacked_beats_unstacked_against_a_direct_fourier_sum(case):
    """err(A) = max|A - I| / max|I| over the inner half of the field, I the direct sum.  Measured with the oracle:
    stacked 0.203 / 0.169 / 0.199, un-stacked 0.421 / 0.898 / 0.436 (ratios 0.48, 0.19, 0.46); the plus-sign screen
    gives 1.44 / 1.26 / 1.26, so the bound 0.75 x un-stacked separates the two signs."""
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
    inner = slice(N // 4, N - N // 4)

    def err(A):
        return np.abs(A[inner, inner] - direct[inner, inner]).max() / np.abs(direct[inner, inner]).max()

    stacked = err(W.Stack(theta, lam, u, v, w, wstep, M, q, ff, S).dirty(vis))
    unstacked = err(R.ifft_c(R.w_cache_imaging(theta, lam, u, v, w, vis, wstep, q, ff, S)[0]))
    plus = err(W.Stack(theta, lam, u, v, w, wstep, M, q, ff, S, sign=+1.0).dirty(vis))
    print(f"N={N} M={M}: stacked {stacked:.4f} un-stacked {unstacked:.4f} ratio {stacked / unstacked:.3f} plus-sign {plus:.4f}")
    assert stacked <= 0.75 * unstacked
    assert plus > 0.75 * unstacked  # (the wrong sign is on the other side of the bound)


# ---- 2: the adjoint identity of the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,lam,M", [(0.1, 320, 3), (0.1, 330, 4)], ids=["N32", "N33"])
def test_restatement_predict_is_the_adjoint_of_image(theta, lam, M):
    rng = np.random.default_rng(7)
    n = 200
    N = W.image_size(theta, lam)
    u, v = rng.uniform(-0.4 * lam, 0.4 * lam, n), rng.uniform(-0.4 * lam, 0.4 * lam, n)
    w = rng.uniform(-900, 900, n)
    w[5] = np.nan  # (a visibility without a layer is in neither map)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    st = W.Stack(theta, lam, u, v, w, 100, M, 2, 16, 7)
    lhs = np.sum(model * st.image(vis))
    rhs = np.real(np.vdot(vis, st.predict(model))) / (N * N)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert st.predict(model)[5] == 0 and st.predict(model, vis_sub=vis)[5] == vis[5]


# ---- 3: M = 1 -----------------------------------------------------------------------------------------------------------------------
def test_one_plane_per_layer():
    theta, lam = 0.1, 320
    w = np.array([-250.0, -49.0, 0.0, 149.0, 151.0, 420.0])
    lay = W.layers(w, 100, 1)
    assert np.all(lay["r"] == 0)
    assert lay["pmin"] == -3 and lay["L"] == 8  # planes -3 .. 4 (round half away: -250 -> -3)
    assert np.array_equal(lay["layer"], [0, 3, 3, 4, 5, 7]) and np.array_equal(lay["pc"], np.arange(-3, 5))
    K = W.kernel_table(theta, 100, 1, 16, 7, 2)
    assert K.shape == (1, 2, 2, 7, 7) and np.array_equal(K[0], np.conj(R.w_kernel(theta, 0.0, 16, 7, 2)))


# ---- 4: the layer arithmetic ----------------------------------------------------------------------------------------------------------
def test_layer_arithmetic():
    # negative planes, odd M: planes -7 .. 3, pmin -7, M 3 -> L = 4, centres -6, -3, 0, 3
    lay = W.layers(np.array([-700.0, -460.0, -10.0, 300.0]), 100, 3)
    assert (lay["pmin"], lay["L"]) == (-7, 4) and np.array_equal(lay["pc"], [-6, -3, 0, 3])
    assert np.array_equal(lay["layer"], [0, 0, 2, 3]) and np.array_equal(lay["r"], [0, 2, 1, 1])  # planes -7 -5 0 3
    # even M: the centre is the upper middle plane, pc = pmin + l M + M div 2; r = p - pmin - l M
    lay = W.layers(np.array([0.0, 100.0, 200.0, 300.0, 400.0]), 100, 4)
    assert (lay["pmin"], lay["L"]) == (0, 2) and np.array_equal(lay["pc"], [2, 6])
    assert np.array_equal(lay["layer"], [0, 0, 0, 0, 1]) and np.array_equal(lay["r"], [0, 1, 2, 3, 0])
    # w exactly at a half-plane tie rounds away from zero, on either side
    lay = W.layers(np.array([50.0, -50.0, 150.0, -150.0, 49.999999999999]), 100, 2)
    assert lay["pmin"] == -2 and np.array_equal(lay["layer"] * 2 + lay["r"] + lay["pmin"], [1, -1, 2, -2, 0])
    # a gap that leaves a layer empty
    lay = W.layers(np.array([0.0, 10.0, 900.0]), 100, 3)
    assert lay["L"] == 4 and sorted(set(lay["layer"])) == [0, 3]
    # one visibility; all visibilities in one plane
    lay = W.layers(np.array([-1234.0]), 100, 5)
    assert (lay["L"], lay["pmin"]) == (1, -12) and lay["layer"][0] == 0 and lay["r"][0] == 0 and lay["pc"][0] == -10
    lay = W.layers(np.full(7, 333.0), 100, 4)
    assert lay["L"] == 1 and np.all(lay["layer"] == 0) and np.all(lay["r"] == 0)
    # n = 0
    lay = W.layers(np.zeros(0), 100, 4)
    assert lay["L"] == 0 and len(lay["layer"]) == 0
    st = W.Stack(0.1, 160, np.zeros(0), np.zeros(0), np.zeros(0), 100, 4, 2, 16, 7)
    assert st.image(np.zeros(0, dtype=c128)).shape == (16, 16) and not st.image(np.zeros(0, dtype=c128)).any()
    # a non-finite w has no layer and does not move pmin / pmax
    lay = W.layers(np.array([np.nan, 100.0, np.inf, 300.0, -np.inf]), 100, 2)
    assert (lay["pmin"], lay["L"]) == (1, 2) and np.array_equal(lay["layer"], [-1, 0, -1, 1, -1])
    assert W.layers(np.array([np.nan, np.inf]), 100, 2)["L"] == 0


# ---- 5: the ABI and the marshalling ------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_stack():
    from gridhip import _lib
    import gridhip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gridhip.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
        assert f'foreign import ccall unsafe "{name}"' in hs, name
    for host in ("gridhip_do_imaging_wstack", "gridhip_predict_wstack"):
        assert _lib.SIGNATURES[host] == _lib.SIGNATURES[host + "_dev"]
    assert callable(gridhip.Context.wstack) and callable(gridhip.WStack.image) and callable(gridhip.WStack.predict)
    assert _lib.load().gridhip_version() >= 300


def test_null_handles_are_refused():
    from gridhip import _lib
    lib = _lib.load()
    x = np.zeros(64)
    p = C.c_void_p(x.ctypes.data)
    h = C.c_void_p(0x1234)
    assert lib.gridhip_wstack_create_dev(None, 100, 2, 2, 16, 7, 0.1, 160, 4, p, p, p, 1, C.byref(h)) == _lib.EINVAL
    assert h.value == 0x1234  # (no context: nothing is touched)
    assert lib.gridhip_wstack_image_dev(None, p, p) == _lib.EINVAL
    assert lib.gridhip_wstack_predict_dev(None, p, None, p) == _lib.EINVAL
    assert lib.gridhip_wstack_info(None, None, None, None, None) == _lib.EINVAL
    assert lib.gridhip_wstack_destroy(None) == _lib.OK
    pm = C.c_double()
    for fn in (lib.gridhip_do_imaging_wstack, lib.gridhip_do_imaging_wstack_dev):
        assert fn(None, 100, 2, 2, 16, 7, 0.1, 160, 4, p, p, p, 1, p, p, p, C.byref(pm)) == _lib.EINVAL
    for fn in (lib.gridhip_predict_wstack, lib.gridhip_predict_wstack_dev):
        assert fn(None, 100, 2, 2, 16, 7, 0.1, 160, p, 4, p, p, p, 1, None, p) == _lib.EINVAL


THETA, LAM, NPIX, NV = 0.008, 2000, 16, 6
OPTS = dict(wstep=40, planes=3, qpx=2, npixFF=8, npixKern=5)


@pytest.fixture
def rig():
    import gridhip
    from test_binding_marshalling import Recorder
    rec = Recorder()
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = rec, HANDLE, 0

    def run(fn, name, *spec):
        before = len(rec.calls)
        rec.expect(name, HANDLE, spec)
        out = fn()
        assert rec.calls[before:] == [name], f"{name}: the calls were {rec.calls[before:]}"
        return out
    yield ctx, rec, run
    ctx._h = None


def stream():
    u = (np.arange(NV, dtype=np.float32) - 2) * 8
    v = (np.arange(2 * NV, dtype=f64))[::2]
    w = [float(k) * 30 - 70 for k in range(NV)]
    vis = (np.arange(NV) - 1j * (np.arange(NV) % 3)).astype(np.complex64)
    return u, v, w, vis


def test_do_imaging_and_predict_reach_the_stack(rig):
    ctx, rec, run = rig
    u, v, w, vis = stream()
    img, psf = Out(f64, NPIX * NPIX), Out(f64, NPIX * NPIX)
    spec = [40, 3, 2, 8, 5, THETA, LAM]
    got = run(lambda: ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("wstack", OPTS)),
              "gridhip_do_imaging_wstack", *spec, NV, Arr(u, f64), Arr(v, f64), Arr(w, f64), 1, Arr(vis, c128), img, psf,
              Ref(C.c_double, 2.5))
    assert img.returned(got[0], (NPIX, NPIX)) and psf.returned(got[1], (NPIX, NPIX)) and got[2] == 2.5
    # the (n, 3) matrix goes at stride 3; no wstep: 2000
    m = np.stack([u, v, w], axis=1).astype(f64)
    flat = m.ravel()
    opts = dict(OPTS, wstep=None)
    run(lambda: ctx.do_imaging(THETA, LAM, m, None, None, None, None, vis, ("wstack", opts)), "gridhip_do_imaging_wstack",
        2000, 3, 2, 8, 5, THETA, LAM, NV, Arr(flat, f64), Arr(flat[1:], f64), Arr(flat[2:], f64), 3, Arr(vis, c128), img, psf,
        Ref(C.c_double, 1.0))
    model = np.arange(NPIX * NPIX, dtype=np.float32).reshape(NPIX, NPIX)
    o = Out(c128, NV)
    got = run(lambda: ctx.predict(THETA, LAM, (u, v, w), model, ("wstack", OPTS)), "gridhip_predict_wstack", *spec,
              Arr(model, f64), NV, Arr(u, f64), Arr(v, f64), Arr(w, f64), 1, None, o)
    assert o.returned(got, (NV,))
    sub = np.arange(NV).astype(c128)
    from test_binding_marshalling import Same
    assert run(lambda: ctx.predict(THETA, LAM, (u, v, w), model, ("wstack", OPTS), vis_sub=sub, out=sub),
               "gridhip_predict_wstack", *spec, Arr(model, f64), NV, Arr(u, f64), Arr(v, f64), Arr(w, f64), 1, Same(sub),
               Same(sub)) is sub


@pytest.mark.parametrize("bad", [dict(planes=0), dict(planes=-2), dict(wstep=-5), dict(npixKern=9), dict(qpx=0),
                                 dict(npixFF=5, npixKern=5, qpx=4)])
def test_bad_options_raise_before_any_call(rig, bad):
    ctx, rec, run = rig
    u, v, w, vis = stream()
    opts = dict(OPTS, **bad)
    model = np.zeros((NPIX, NPIX))
    with pytest.raises(ValueError):
        ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("wstack", opts))
    with pytest.raises(ValueError):
        ctx.predict(THETA, LAM, (u, v, w), model, ("wstack", opts))
    with pytest.raises(ValueError):
        ctx.wstack(THETA, LAM, (u, v, w), opts)
    assert rec.calls == []


def test_missing_planes_and_a_wrong_model_shape_raise_before_any_call(rig):
    ctx, rec, run = rig
    u, v, w, vis = stream()
    no_planes = {k: x for k, x in OPTS.items() if k != "planes"}
    with pytest.raises(KeyError):
        ctx.do_imaging(THETA, LAM, (u, v, w), None, None, None, None, vis, ("wstack", no_planes))
    with pytest.raises(ValueError):
        ctx.predict(THETA, LAM, (u, v, w), np.zeros((NPIX, NPIX + 1)), ("wstack", OPTS))
    assert rec.calls == []
