"""Gain calibration (gridhip_gaincal*, gridhip_apply_gains*, gridhip_imager_selfcal_dev), the checks that need no GPU: the
library, the header, the ctypes table, both bindings and the hpp carry the five entry points; a NULL context or imager is
refused with GRIDHIP_EINVAL whatever else is passed; Context.gaincal and Context.apply_gains hand the ABI the right
pointers, scalar order and NULL for slot=None / weights=None (against the recording library of
test_binding_marshalling.py) and refuse wrong dtypes and shapes before any call; and the numpy restatement the GPU tests
compare with (tests/gaincal_ref.py) is right on cases computed by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gaincal_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_gaincal", "gridhip_gaincal_dev", "gridhip_apply_gains", "gridhip_apply_gains_dev",
         "gridhip_imager_selfcal_dev"]
f64, c128, i64 = np.float64, np.complex128, np.int64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_five():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_gaincal"] == _lib.SIGNATURES["gridhip_gaincal_dev"]
    assert _lib.SIGNATURES["gridhip_apply_gains"] == _lib.SIGNATURES["gridhip_apply_gains_dev"]
    assert _lib.load().gridhip_version() >= 210
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 210
    # the semantics are stated in the header: the limit, the determinism, the classes
    for phrase in ("GRIDHIP_EUNSUPPORTED", "2^21", "DETERMINISM", "FLAGGED", "DROPPED", "AUTO", "UNSOLVED"):
        assert phrase in raw[raw.index("gain calibration"):raw.index("int gridhip_gaincal(")], phrase


def test_bindings_carry_the_five():
    import gridhip
    for owner, method in ((gridhip.Context, "gaincal"), (gridhip.Context, "apply_gains"), (gridhip.Imager, "selfcal")):
        assert callable(getattr(owner, method)), method
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("gaincalIO", "applyGainsIO", "imagerSelfcalIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bgaincal\s*\(", hpp) and re.search(r"\bapply_gains\s*\(", hpp)
    for name in NAMES:
        assert name in hpp, name


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_gaincal.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    n, A, T = 3, 3, 1
    a1, a2, sl = np.array([0, 0, 1], dtype=i64), np.array([1, 2, 2], dtype=i64), np.zeros(n, dtype=i64)
    vis, mod, out = np.full(n, 1 + 2j), np.full(n, 3 + 0j), np.full(n, 7 + 7j)
    wt, wo, g, st = np.full(n, 4.0), np.full(n, 8.0), np.full((T, A), 5 + 5j), np.full(8, 6.0)
    p1, p2, ps, pv, pm, po, pw, pwo, pg, pst = (C.c_void_p(a.ctypes.data) for a in (a1, a2, sl, vis, mod, out, wt, wo, g, st))
    for fn in (lib.gridhip_gaincal, lib.gridhip_gaincal_dev):
        for (nn, AA, TT, slot, mode, ref, niter, tol) in [
                (n, A, T, ps, 0, 0, 5, 1e-8), (n, A, T, None, 1, -1, 0, 0.0), (-1, A, T, ps, 0, 0, 5, 0.0),
                (n, 1, T, ps, 0, 0, 5, 0.0), (n, A, 0, ps, 0, 0, 5, 0.0), (n, A, 2, None, 0, 0, 5, 0.0),
                (n, A, T, ps, 2, 0, 5, 0.0), (n, A, T, ps, 0, A, 5, 0.0), (n, A, T, ps, 0, 0, -1, 0.0),
                (n, A, T, ps, 0, 0, 5, -1.0), (n, A, T, ps, 0, 0, 5, float("nan")), (n, 1 << 11, 1 << 11, ps, 0, 0, 1, 0.0)]:
            assert fn(None, nn, AA, TT, p1, p2, slot, pv, pm, pw, mode, ref, 0, niter, tol, pg, pst) == _lib.EINVAL
            assert fn(None, nn, AA, TT, p1, p2, slot, pv, pm, None, mode, ref, 1, niter, tol, pg, None) == _lib.EINVAL
        assert fn(None, n, A, T, p1, p2, ps, None, pm, pw, 0, 0, 0, 5, 0.0, None, pst) == _lib.EINVAL
        assert fn(None, n, A, T, p1, p2, ps, pv, pm, pw, 0, 0, 0, 5, 0.0, pv, pst) == _lib.EINVAL  # gains over vis
    for fn in (lib.gridhip_apply_gains, lib.gridhip_apply_gains_dev):
        for inverse in (1, 0, 2, -1):
            assert fn(None, n, A, T, p1, p2, ps, pg, inverse, pv, pw, po, pwo) == _lib.EINVAL
            assert fn(None, n, A, T, p1, p2, None, pg, inverse, pv, None, pv, None) == _lib.EINVAL  # in place
        assert fn(None, n, A, T, p1, p2, ps, pg, 1, pv, pw, pg, pwo) == _lib.EINVAL  # vis_out over gains
        assert fn(None, n, 1, T, None, p2, ps, None, 1, pv, pw, None, pwo) == _lib.EINVAL
    for mode in (0, 1, 5):
        assert lib.gridhip_imager_selfcal_dev(None, pwo, pv, A, T, p1, p2, ps, pw, mode, 0, 0, 5, 1e-8, pg, po, pwo,
                                              pst) == _lib.EINVAL
        assert lib.gridhip_imager_selfcal_dev(None, None, None, 1, 0, None, None, None, None, mode, 9, 0, -1, -1.0, None,
                                              None, None, None) == _lib.EINVAL
    for a, val in ((vis, 1 + 2j), (mod, 3 + 0j), (out, 7 + 7j), (wt, 4.0), (wo, 8.0), (g, 5 + 5j), (st, 6.0)):
        assert np.all(a == val)


# ---- marshalling: what Context.gaincal and Context.apply_gains hand to the ABI ------------------------------------------
@pytest.fixture
def rig():
    import gridhip
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


N = 6
A1, A2 = [0, 1, 2, 0, 1, 2], np.array([2, 2, 0, 1, 0, 1], dtype=np.int32)
SLOT = np.array([0, 0, 0, 1, 1, 1], dtype=np.int16)


def awkward_vis():
    vis = (np.arange(2 * N) * (1 - 0.5j)).astype(c128)[::2]  # not contiguous
    mod = (np.arange(N) + 1j).astype(np.complex64)
    assert not vis.flags.c_contiguous
    return vis, mod


def test_gaincal_marshalling(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    wt = np.arange(N, dtype=np.float32)
    g_out, st_out = Out(c128, 2 * 3), Out(f64, 8)
    g, st = run(lambda: ctx.gaincal(vis, mod, A1, A2, 3, slot=SLOT, nslots=2, weights=wt, phase_only=True, refant=None,
                                    niter=7, tol=1e-6),
                "gridhip_gaincal", N, 3, 2, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(vis, c128), Arr(mod, c128),
                Arr(wt, f64), 1, -1, 0, 7, 1e-6, g_out, st_out)
    assert g_out.returned(g, (2, 3)) and st_out.returned(st, (8,))
    # slot=None and weights=None are NULL; arrays already in the ABI's form go by their own address; a given gains is the
    # warm start, updated in place and returned
    v2, m2 = np.ascontiguousarray(vis), np.ascontiguousarray(mod, dtype=c128)
    a1, a2 = np.array(A1, dtype=i64), np.array(A2, dtype=i64)
    warm = np.ones((1, 3), dtype=c128)
    g, st = run(lambda: ctx.gaincal(v2, m2, a1, a2, 3, gains=warm),
                "gridhip_gaincal", N, 3, 1, Same(a1), Same(a2), None, Same(v2), Same(m2), None, 0, 0, 1, 50, 1e-8,
                Same(warm), Out(f64, 8))
    assert g is warm


def test_apply_gains_marshalling(rig):
    ctx, rec, run = rig
    vis, _ = awkward_vis()
    gains = (np.arange(6).reshape(2, 3) + 2j).astype(np.complex64)
    wt = np.arange(N, dtype=f64)
    o, w = Out(c128, N), Out(f64, N)
    vo, wo = run(lambda: ctx.apply_gains(gains, vis, A1, A2, slot=SLOT, weights=wt),
                 "gridhip_apply_gains", N, 3, 2, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(gains, c128), 1,
                 Arr(vis, c128), Same(wt), o, w)
    assert o.returned(vo, (N,)) and w.returned(wo, (N,))
    # one interval, no weights, corrupting a model, in place
    g1, v2 = np.ones((1, 3), dtype=c128), np.ascontiguousarray(vis)
    wout = np.zeros(N)
    vo, wo = run(lambda: ctx.apply_gains(g1, v2, A1, A2, inverse=False, out=v2, weights_out=wout),
                 "gridhip_apply_gains", N, 3, 1, Arr(A1, i64), Arr(A2, i64), None, Same(g1), 0, Same(v2), None, Same(v2),
                 Same(wout))
    assert vo is v2 and wo is wout


def test_wrong_dtypes_and_shapes_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    ok = dict(vis=vis, model_vis=mod, a1=A1, a2=A2, nant=3)
    bad = [dict(a1=np.array(A1, dtype=f64)), dict(a2=A2[:-1]), dict(model_vis=mod[:-1]), dict(vis=np.zeros((N, 1), dtype=c128)),
           dict(slot=SLOT.astype(np.float32), nslots=2), dict(slot=SLOT[:-1], nslots=2), dict(nslots=2), dict(nant=1),
           dict(nslots=0, slot=SLOT), dict(weights=np.ones(N - 1)), dict(weights=np.ones(N, dtype=c128)),
           dict(gains=np.ones((1, 3), dtype=np.complex64)), dict(gains=np.ones((3, 1), dtype=c128)),
           dict(gains=np.ones((1, 6), dtype=c128)[:, ::2]), dict(refant=3), dict(niter=-1), dict(tol=-1.0),
           dict(tol=float("nan"))]
    for change in bad:
        with pytest.raises(ValueError):
            ctx.gaincal(**{**ok, **change})
    g = np.ones((2, 3), dtype=c128)
    for kw in [dict(gains=np.ones(3, dtype=c128)), dict(a1=np.array(A1, dtype=f64)), dict(slot=None),
               dict(out=np.zeros(N, dtype=np.complex64)), dict(out=np.zeros(N + 1, dtype=c128)),
               dict(weights_out=np.zeros(N, dtype=np.float32)), dict(weights=np.ones(N + 1))]:
        args = {**dict(gains=g, vis=vis, a1=A1, a2=A2, slot=SLOT), **kw}
        with pytest.raises(ValueError):
            ctx.apply_gains(args.pop("gains"), args.pop("vis"), args.pop("a1"), args.pop("a2"), **args)
    assert rec.calls == []


# ---- the numpy restatement on cases computed by hand ---------------------------------------------------------------------
def test_one_iteration_from_unity_is_sum_x_over_sum_y():
    """Three antennas, the three baselines, g = 1: num[a] = sum of X over the baselines with p = a plus conj(X) over those
    with q = a, den[a] = the sum of Y over both."""
    a1, a2 = np.array([0, 0, 1]), np.array([1, 2, 2])
    V, M, s = np.array([2 + 1j, 1 - 3j, -1 + 0.5j]), np.array([1 + 1j, 2 + 0j, 0.5 - 1j]), np.array([1.0, 2.0, 0.5])
    X, Y = s * V * np.conj(M), s * np.abs(M) ** 2
    want = np.array([(X[0] + X[1]) / (Y[0] + Y[1]), (np.conj(X[0]) + X[2]) / (Y[0] + Y[2]),
                     (np.conj(X[1]) + np.conj(X[2])) / (Y[1] + Y[2])])
    g, st = gaincal_ref.gaincal(V, M, a1, a2, 3, wt=s, refant=-1, niter=1, tol=0)
    assert np.allclose(g[0], want, rtol=1e-15, atol=0)
    assert list(st[[0, 4, 5, 6, 7]]) == [1, 3, 0, 0, 0]
    assert st[1] == pytest.approx(np.sqrt((np.abs(want - 1) ** 2).sum() / (np.abs(want) ** 2).sum()), rel=1e-14)
    assert st[3] == pytest.approx((s * np.abs(V - M) ** 2).sum(), rel=1e-14)
    # phase only: the same direction, unit modulus
    gp, _ = gaincal_ref.gaincal(V, M, a1, a2, 3, wt=s, mode=1, refant=-1, niter=1, tol=0)
    assert np.allclose(gp[0], want / np.abs(want), rtol=1e-15, atol=0)
    # the second iteration (i = 1, odd) is averaged with the first
    g2, _ = gaincal_ref.gaincal(V, M, a1, a2, 3, wt=s, refant=-1, niter=2, tol=0)
    num = np.array([X[0] * g[0, 1] + X[1] * g[0, 2], np.conj(X[0]) * g[0, 0] + X[2] * g[0, 2],
                    np.conj(X[1]) * g[0, 0] + np.conj(X[2]) * g[0, 1]])
    den = np.array([Y[0] * abs(g[0, 1]) ** 2 + Y[1] * abs(g[0, 2]) ** 2, Y[0] * abs(g[0, 0]) ** 2 + Y[2] * abs(g[0, 2]) ** 2,
                    Y[1] * abs(g[0, 0]) ** 2 + Y[2] * abs(g[0, 1]) ** 2])
    assert np.allclose(g2[0], (num / den + g[0]) / 2, rtol=1e-14, atol=0)


def corrupted(rng, A, T, reps=2, noise=0.0):
    p, q = np.triu_indices(A, 1)
    a1, a2 = np.tile(p, T * reps), np.tile(q, T * reps)
    sl = np.repeat(np.arange(T), len(p) * reps)
    n = len(a1)
    M = rng.normal(size=n) + 1j * rng.normal(size=n) + 3
    gt = (1 + 0.3 * rng.normal(size=(T, A))) * np.exp(1j * rng.uniform(-2, 2, (T, A)))
    V = gt[sl, a1] * M * np.conj(gt[sl, a2]) + noise * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return a1, a2, sl, V, M, rng.uniform(0.5, 2, n), gt


@pytest.mark.parametrize("A,T", [(3, 1), (7, 3)])
def test_noise_free_recovery_up_to_the_reference_phase(A, T):
    a1, a2, sl, V, M, w, gt = corrupted(np.random.default_rng(1), A, T)
    g, st = gaincal_ref.gaincal(V, M, a1, a2, A, slot=sl, T=T, wt=w, refant=0, niter=200, tol=1e-12)
    truth = gt * np.exp(-1j * np.angle(gt[:, :1]))
    assert st[0] < 200 and st[1] <= 1e-12
    assert np.abs(g - truth).max() < 1e-10
    assert np.all(g[:, 0].imag == 0) and np.all(g[:, 0].real > 0)
    assert st[2] < 1e-18 * st[3] and st[7] == 0
    # phase only, on data corrupted by phases alone
    ph = gt / np.abs(gt)
    Vp = ph[sl, a1] * M * np.conj(ph[sl, a2])
    g, st = gaincal_ref.gaincal(Vp, M, a1, a2, A, slot=sl, T=T, wt=w, mode=1, refant=0, niter=200, tol=1e-12)
    assert st[0] < 60 and np.abs(g - ph * np.exp(-1j * np.angle(ph[:, :1]))).max() < 1e-10
    assert np.abs(np.abs(g) - 1).max() < 1e-15
    # and apply(inverse) with the solved gains gives the model back; corrupting the model gives the data
    back, wout = gaincal_ref.apply_gains(g, Vp, a1, a2, slot=sl, wt=w)
    assert np.abs(back - M).max() < 1e-9 and np.allclose(wout, w, rtol=1e-14)
    fwd, wf = gaincal_ref.apply_gains(g, M, a1, a2, slot=sl, wt=w, inverse=False)
    assert np.abs(fwd - Vp).max() < 1e-9 and np.array_equal(wf, w)


def test_flagged_nan_changes_nothing_and_dropped_are_counted():
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(2), 4, 2, noise=0.05)
    g0, st0 = gaincal_ref.gaincal(V, M, a1, a2, 4, slot=sl, T=2, wt=w, niter=6, tol=0)
    extra = 5
    a1x, a2x = np.concatenate([a1, [0, 1, 9, 2, 2]]), np.concatenate([a2, [1, 2, 1, -1, 2]])
    slx = np.concatenate([sl, [0, 1, 0, 0, 1]])
    Vx = np.concatenate([V, [np.nan, np.inf, 1, 1, 1]])
    Mx = np.concatenate([M, [1, np.nan + 1j * np.inf, 1, 1, 1]])
    wx = np.concatenate([w, [0.0, np.nan, 1.0, 1.0, 1.0]])  # two flagged, two out of range, one autocorrelation
    order = np.random.default_rng(3).permutation(len(a1) + extra)
    g1, st1 = gaincal_ref.gaincal(Vx[order], Mx[order], a1x[order], a2x[order], 4, slot=slx[order], T=2, wt=wx[order],
                                  niter=6, tol=0)
    assert np.abs(g1 - g0).max() < 1e-13
    assert list(st1[4:]) == [st0[4], 2, 3, 0] and np.allclose(st1[:4], st0[:4], rtol=1e-12)
    # a negative weight flags too; a slot out of range drops
    _, st = gaincal_ref.gaincal(V[:3], M[:3], [0, 0, 1], [1, 2, 2], 4, slot=[0, 2, -1], T=2, wt=[-1.0, 1.0, 1.0], niter=1)
    assert list(st[4:]) == [0, 1, 2, 8]


def test_two_antennas_recover_the_product_and_not_the_factors():
    rng = np.random.default_rng(4)
    n = 8
    M = rng.normal(size=n) + 1j * rng.normal(size=n) + 2
    gt = np.array([1.3 * np.exp(0.7j), 0.6 * np.exp(-1.1j)])
    V = gt[0] * M * np.conj(gt[1])
    g, st = gaincal_ref.gaincal(V, M, np.zeros(n, dtype=int), np.ones(n, dtype=int), 2, refant=0, niter=200, tol=1e-13)
    assert abs(g[0, 0] * np.conj(g[0, 1]) - gt[0] * np.conj(gt[1])) < 1e-11
    assert abs(abs(g[0, 0]) - abs(g[0, 1])) < 1e-9  # (from g = 1 the iteration splits the modulus evenly)
    assert abs(abs(g[0, 0]) - 1.3) > 0.1 and g[0, 0].imag == 0


def test_unsolved_and_niter_zero():
    V, M = np.array([1 + 1j, 2 + 0j]), np.array([1 + 0j, 1 + 0j])
    warm = np.array([[2j, 1 + 1j, 3 + 0j, 0.5j], [1, 1, 1, 1]], dtype=c128)
    g, st = gaincal_ref.gaincal(V, M, [0, 0], [1, 1], 4, slot=[0, 0], T=2, gains=warm, refant=2, niter=0)
    assert np.array_equal(g, warm) and list(st[[0, 4, 7]]) == [0, 2, 8] and np.isnan(st[1])
    # antennas 2, 3 and interval 1 have no data: their gains stay the warm bits; refant 2 is unsolved: nothing is rotated
    g, st = gaincal_ref.gaincal(V, M, [0, 0], [1, 1], 4, slot=[0, 0], T=2, gains=warm, refant=2, niter=3, tol=0)
    assert np.array_equal(g[0, 2:], warm[0, 2:]) and np.array_equal(g[1], warm[1]) and st[7] == 6
    assert g[0, 0].imag != 0 and st[0] == 3
    # apply: a zero or NaN gain and an index out of range give weight +0.0 and the visibility unchanged
    gz = np.array([[1 + 1j, 0, np.nan, 2]], dtype=c128)
    out, wout = gaincal_ref.apply_gains(gz, [1 + 2j] * 5, [0, 0, 0, 0, 3], [3, 1, 2, 4, 0], wt=[2.0] * 5)
    assert list(out[1:4]) == [1 + 2j] * 3 and list(wout[1:4]) == [0.0] * 3 and not np.signbit(wout[1:4]).any()
    assert out[0] == (1 + 2j) / ((1 + 1j) * 2) and wout[0] == 2.0 * 2.0 * 4.0
    assert out[4] == (1 + 2j) / (2 * (1 - 1j))
