"""Wide-band imaging (gridhip_mfclean*, gridhip_imager_set_spectral_dev, _spectral_psfs_dev, _mfs_cycle_dev, _mfclean_dev,
_mfdeconvolve_dev), the checks that need no GPU: the library, the header, the ctypes table, both bindings and the hpp carry
the entry points; a NULL context or imager is refused with GRIDHIP_EINVAL; every new Python method hands the ABI the right
pointers, plane counts, scalar order and stats buffer (against the recording library of test_binding_marshalling.py) and
refuses wrong dtypes and shapes before any call; and the numpy restatement the GPU tests compare with
(tests/mfclean_ref.py) is right on a case computed by hand and, for one term, is the Hogbom restatement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clean_ref
import mfclean_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Same
from test_clean_host import SameT, Zeros, rig, tensor_returned, torch_rig  # noqa: F401  (rig, torch_rig: fixtures)

NAMES = ["gridhip_mfclean", "gridhip_mfclean_dev", "gridhip_imager_set_spectral_dev", "gridhip_imager_spectral_psfs_dev",
         "gridhip_imager_mfs_cycle_dev", "gridhip_imager_mfclean_dev", "gridhip_imager_mfdeconvolve_dev"]
f64 = np.float64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_entry_points():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_mfclean"] == _lib.SIGNATURES["gridhip_mfclean_dev"]
    assert _lib.load().gridhip_version() >= 200
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 200
    assert "wide-band imaging" in raw


def test_bindings_carry_the_entry_points():
    import gridhip
    assert callable(gridhip.Context.mfclean)
    for m in ("set_spectral", "spectral_psfs", "mfs_cycle", "mfclean", "mfdeconvolve"):
        assert callable(getattr(gridhip.Imager, m)), m
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("mfcleanIO", "imagerMfsCycleIO", "imagerMfDeconvolveIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bmfclean\s*\(", hpp) and "gridhip_mfclean" in hpp


def test_null_handles_are_refused_and_nothing_is_touched():
    from gridhip import _lib
    lib = _lib.load()
    N, T = 4, 2
    psfs, res, mod = np.full(3 * N * N, 1.0), np.full(T * N * N, 2.0), np.full(T * N * N, 3.0)
    vis, stats = np.full(2 * 5, 4.0), np.full(16, 7.0)
    p, r, m, v, s = (C.c_void_p(a.ctypes.data) for a in (psfs, res, mod, vis, stats))
    for sc in [(0.1, 0.0, 5, 0, 0), (0.0, 0.0, 5, 0, 0), (0.1, -1.0, 5, 0, 0), (0.1, 0.0, -1, 0, 0), (0.1, 0.0, 5, 2, 0)]:
        for t in (T, 0, 5):
            assert lib.gridhip_mfclean(None, N, t, p, r, m, *sc, s) == _lib.EINVAL
            assert lib.gridhip_mfclean_dev(None, N, t, p, r, m, *sc, s) == _lib.EINVAL
        assert lib.gridhip_imager_mfclean_dev(None, r, m, *sc, s) == _lib.EINVAL
        assert lib.gridhip_imager_mfdeconvolve_dev(None, v, m, r, 2, *sc, s) == _lib.EINVAL
    assert lib.gridhip_imager_set_spectral_dev(None, T, v) == _lib.EINVAL
    assert lib.gridhip_imager_spectral_psfs_dev(None, p) == _lib.EINVAL
    assert lib.gridhip_imager_mfs_cycle_dev(None, m, v, r, None) == _lib.EINVAL
    for a, val in ((psfs, 1.0), (res, 2.0), (mod, 3.0), (vis, 4.0), (stats, 7.0)):
        assert np.all(a == val)


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
def hand_case():
    """N = 5, c = (2, 2), T = 2.  P_0: 1 at the centre, 0.5 at its four neighbours; P_1 = P_2 = 0.5 at the centre alone.
    H = [[1, .5], [.5, .5]]; the elimination: row 0 / 1; row 1 - .5 row 0 = [0, .25 | -.5, 1]; row 1 / .25 = [0, 1 | -2, 4];
    row 0 - .5 row 1 = [1, 0 | 2, -2]: Hinv = [[2, -2], [-2, 4]], all exact.
    A source I_0 = 2, I_1 = 4 at (3, 1): R_0 = 2 P_0 + 4 P_1, R_1 = 2 P_1 + 4 P_2 shifted there - at the source cell
    R = (4, 3), at its four neighbours R = (1, 0)."""
    psfs = np.zeros((3, 5, 5))
    psfs[0][2, 2] = 1.0
    psfs[0][1, 2] = psfs[0][3, 2] = psfs[0][2, 1] = psfs[0][2, 3] = 0.5
    psfs[1][2, 2] = psfs[2][2, 2] = 0.5
    res = np.zeros((2, 5, 5))
    res[0][3, 1], res[1][3, 1] = 4.0, 3.0
    for y, x in ((2, 1), (4, 1), (3, 0), (3, 2)):
        res[0][y, x] = 1.0
    return psfs, res


def test_restatement_on_a_hand_computed_case():
    psfs, res = hand_case()
    Hinv, ok = mfclean_ref.invert([[1.0, 0.5], [0.5, 0.5]])
    assert ok and Hinv == [[2.0, -2.0], [-2.0, 4.0]]
    # at the source a = (2 * 4 - 2 * 3, -2 * 4 + 4 * 3) = (2, 4), s = 2 * 4 + 4 * 3 = 20; at a neighbour a = (2, -2), s = 2:
    # k = 16, p = 2, the gap (20 - 2) / 20; gain 0.5: f = (1, 2), and exactly half of the source remains
    models, trace = np.zeros((2, 5, 5)), []
    start = res.copy()
    st = mfclean_ref.mfclean(psfs, res, models, 0.5, 0.0, 1, trace=trace)
    assert trace == [(16, 0.9)]
    assert np.array_equal(res, 0.5 * start)
    assert models[0][3, 1] == 1.0 and models[1][3, 1] == 2.0 and np.count_nonzero(models) == 2
    assert np.array_equal(st, [1.0, 1.0, 16.0, 1.0, 2.0, 0.0, 0.0, 0.0])
    # gain 1 takes all of it: the coefficients are the source's (I_0, I_1); the final peak is the first zero cell
    res2, models2 = start.copy(), np.zeros((2, 5, 5))
    st = mfclean_ref.mfclean(psfs, res2, models2, 1.0, 0.0, 1)
    assert not res2.any() and models2[0][3, 1] == 2.0 and models2[1][3, 1] == 4.0
    assert np.array_equal(st, [1.0, 0.0, 0.0, 2.0, 4.0, 0.0, 0.0, 1.0])  # (|0| <= 0: the threshold's reason)
    # the threshold is tested on p = a_0 before anything is subtracted (reason 1); niter = 0 reports the peak (reason 0)
    res3, models3 = start.copy(), np.zeros((2, 5, 5))
    assert np.array_equal(mfclean_ref.mfclean(psfs, res3, models3, 0.5, 2.0, 9), [0.0, 2.0, 16.0, 0, 0, 0, 0, 1.0])
    assert np.array_equal(mfclean_ref.mfclean(psfs, res3, models3, 0.5, 0.0, 0), [0.0, 2.0, 16.0, 0, 0, 0, 0, 0.0])
    assert np.array_equal(res3, start) and not models3.any()
    # the border hides nothing here but the neighbour (3, 0); a NaN in either term is never selected; all NaN: reason 2
    res3[1][3, 1] = np.nan
    st = mfclean_ref.mfclean(psfs, res3, models3, 0.5, 0.0, 0, border=1)
    assert st[1] == 2.0 and st[2] == 11.0 and st[7] == 0.0  # the neighbours (2, 1) and (3, 2) tie: the lowest index
    st = mfclean_ref.mfclean(psfs, np.full((2, 5, 5), np.nan), models3, 0.5, 0.0, 3)
    assert np.isnan(st[1]) and st[2] == -1.0 and st[7] == 2.0 and st[0] == 0.0
    # a singular Hessian: nothing is done, reason 3
    sing = np.stack([psfs[0]] * 3)
    res4 = start.copy()
    st = mfclean_ref.mfclean(sing, res4, models3, 0.5, 0.0, 3)
    assert st[7] == 3.0 and st[0] == 0.0 and np.isnan(st[1]) and st[2] == -1.0 and np.array_equal(res4, start)
    assert not mfclean_ref.invert([[0.0]])[1] and not mfclean_ref.invert([[float("nan")]])[1]
    assert not mfclean_ref.invert([[-1.0]])[1]


@pytest.mark.parametrize("border,patch", [(0, 0), (8, 10)])
def test_one_term_is_hogbom_bit_for_bit(border, patch):
    N = 64
    psf = clean_ref.make_psf(N, 100)
    img, _ = clean_ref.make_sky(psf, 200)
    assert np.array_equal(mfclean_ref.make_psfs(N, 100, 1)[0], psf)
    kw = dict(gain=0.2, threshold=0.0, niter=80, border=border, patch=patch)
    r1, m1, t1 = img.copy(), np.zeros_like(img), []
    s1 = clean_ref.clean(psf, r1, m1, trace=t1, **kw)
    r2, m2, t2 = img[None].copy(), np.zeros((1, N, N)), []
    s2 = mfclean_ref.mfclean(psf[None], r2, m2, trace=t2, **kw)
    assert [k for k, _ in t1] == [k for k, _ in t2] and len(t1) == 80
    assert np.array_equal(r1, r2[0]) and np.array_equal(m1, m2[0])
    assert np.array_equal(s2, [s1[0], s1[1], s1[2], s1[3], 0.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("patch", [0, 32])
@pytest.mark.parametrize("wide_border", [False, True])
@pytest.mark.parametrize("N", [256, 255])
def test_four_terms_meet_the_gpu_tests_preconditions(N, wide_border, patch):
    """tests/test_gpu_mfclean.py's T = 4 cases, the restatement alone: the midway threshold stops the loop after some
    components and before niter, threshold 0 is never reached, and the two largest scores never come closer than 1e-8."""
    T, niter, border = 4, 200, N // 8 if wide_border else 0
    psfs = mfclean_ref.make_psfs(N, 100, T)
    img, _ = mfclean_ref.make_sky(psfs, 101)
    mid = mfclean_ref.midway_threshold(psfs, img, border, patch)
    assert mid > 0.0
    for threshold in (mid, 0.0):
        trace = []
        st = mfclean_ref.mfclean(psfs, img.copy(), np.zeros_like(img), 0.2, threshold, niter, border, patch, trace)
        print(f"N {N} border {border} patch {patch} threshold {threshold:.3e}: {st[0]:.0f} components, reason {st[7]:.0f}, "
              f"smallest gap {min(g for _, g in trace):.2e}")
        assert (0 < st[0] < niter and st[7] == 1) if threshold > 0.0 else (st[0] == niter and st[7] == 0), st
        assert len(trace) == st[0] and min(g for _, g in trace) > 1e-8


# ---- what the Python methods hand to the ABI ------------------------------------------------------------------------------
def test_context_mfclean_host_form(rig):  # noqa: F811
    ctx, rec, run = rig
    N, T = 6, 2
    images = np.arange(T * N * N, dtype=f64).reshape(T, N, N)
    psfs = np.arange(3 * N * N, dtype=np.float32).reshape(3, N, N)  # float32: converted
    models = np.ones((T, N, N))
    st = Out(f64, 8)
    m, r, s = run(lambda: ctx.mfclean(images, psfs, gain=0.25, threshold=0.5, niter=7, border=1, patch=2, models=models),
                  "gridhip_mfclean", N, T, Arr(psfs, f64), Same(images), Same(models), 0.25, 0.5, 7, 1, 2, st)
    assert m is models and r is images and st.returned(s, (8,))
    z, st = Zeros(T * N * N), Out(f64, 8)
    m, r, s = run(lambda: ctx.mfclean(images, psfs), "gridhip_mfclean", N, T, Arr(psfs, f64), Same(images), z,
                  0.1, 0.0, 100, 0, 0, st)
    assert r is images and z.out.returned(m, (T, N, N)) and st.returned(s, (8,))
    one = np.zeros((1, N, N))
    right = np.zeros((1, N, N))
    run(lambda: ctx.mfclean(one, right, 1, 2, 3.0, 1, 0, None), "gridhip_mfclean", N, 1, Same(right), Same(one),
        Zeros(N * N), 1.0, 2.0, 3, 1, 0, Out(f64, 8))
    before = len(rec.calls)
    bad = [
        lambda: ctx.mfclean(images.astype(np.float32), psfs),            # updated in place: no conversion
        lambda: ctx.mfclean(images[0], psfs),                            # not a stack
        lambda: ctx.mfclean(np.zeros((5, N, N)), np.zeros((9, N, N))),   # T = 5
        lambda: ctx.mfclean(np.zeros((0, N, N)), np.zeros((0, N, N))),   # T = 0
        lambda: ctx.mfclean(np.zeros((T, N, N + 1)), psfs),              # not square
        lambda: ctx.mfclean(images, psfs[:2]),                           # 2T - 1 PSFs are needed
        lambda: ctx.mfclean(images, np.zeros((3, N + 1, N + 1))),
        lambda: ctx.mfclean(images, psfs, models=np.zeros((T, N, N), dtype=np.float32)),
        lambda: ctx.mfclean(images, psfs, models=np.zeros((1, N, N))),
        lambda: ctx.mfclean(np.zeros((T, N, 2 * N))[:, :, ::2], psfs),   # not contiguous
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"


def test_context_mfclean_device_form(torch_rig):  # noqa: F811
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, T = 6, 3
    images = torch.arange(T * N * N, dtype=torch.float64).reshape(T, N, N)
    psfs32 = torch.arange(5 * N * N, dtype=torch.float32).reshape(5, N, N)
    models = torch.ones((T, N, N), dtype=torch.float64)
    st = Out(f64, 8)
    m, r, s = run(lambda: ctx.mfclean(images, psfs32, 0.25, 0.5, 7, 1, 2, models), "gridhip_mfclean_dev", N, T,
                  Arr(psfs32.numpy(), f64), SameT(images), SameT(models), 0.25, 0.5, 7, 1, 2, st)
    assert m is models and r is images and tensor_returned(st, s, (8,)) and bound == [ctx]
    for call in (lambda: ctx.mfclean(images.to(torch.float32), psfs32), lambda: ctx.mfclean(images, psfs32[:4]),
                 lambda: ctx.mfclean(images, psfs32, models=np.zeros((T, N, N)))):
        with pytest.raises(ValueError):
            call()
    assert rec.calls.count("gridhip_mfclean_dev") == 1


def test_imager_wide_band_methods(torch_rig):  # noqa: F811
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, n, h, T = im.N, im.n, im._h, 2
    x = torch.linspace(-0.2, 0.2, n, dtype=torch.float64)
    x32 = x.to(torch.float32)
    run(lambda: im.set_spectral(x, T), "gridhip_imager_set_spectral_dev", T, SameT(x), handle=h)
    assert im.nterms == T
    run(lambda: im.set_spectral(x32, 3), "gridhip_imager_set_spectral_dev", 3, Arr(x32.numpy(), f64), handle=h)
    assert im.nterms == 3
    run(lambda: im.set_spectral(x), "gridhip_imager_set_spectral_dev", 2, SameT(x), handle=h)
    assert im.nterms == T
    o = Out(f64, 3 * N * N)
    assert tensor_returned(o, run(lambda: im.spectral_psfs(), "gridhip_imager_spectral_psfs_dev", o, handle=h), (3, N, N))

    vis = torch.arange(n, dtype=torch.float64).to(torch.complex128)
    res = torch.zeros(n, dtype=torch.complex128)
    models = torch.ones((T, N, N), dtype=torch.float64)
    images = torch.arange(T * N * N, dtype=torch.float64).reshape(T, N, N)
    o = Out(f64, T * N * N)
    out = run(lambda: im.mfs_cycle(vis), "gridhip_imager_mfs_cycle_dev", None, SameT(vis), o, None, handle=h)
    assert tensor_returned(o, out, (T, N, N))
    out = run(lambda: im.mfs_cycle(vis, models, out=images, vis_res=res), "gridhip_imager_mfs_cycle_dev", SameT(models),
              SameT(vis), SameT(images), SameT(res), handle=h)
    assert out is images
    st = Out(f64, 8)
    m, r, s = run(lambda: im.mfclean(images, models, 0.25, 0.5, 7, 1, 2), "gridhip_imager_mfclean_dev", SameT(images),
                  SameT(models), 0.25, 0.5, 7, 1, 2, st, handle=h)
    assert m is models and r is images and tensor_returned(st, s, (8,))
    z, st = Zeros(T * N * N), Out(f64, 8)
    m, r, s = run(lambda: im.mfclean(images), "gridhip_imager_mfclean_dev", SameT(images), z, 0.1, 0.0, 100, 0, 0, st,
                  handle=h)
    assert tensor_returned(z.out, m, (T, N, N)) and r is images
    st, oi = Out(f64, 3 * 8), Out(f64, T * N * N)
    m, img, s = run(lambda: im.mfdeconvolve(vis, 3, models=models, gain=0.25, threshold=0.5, niter=7, border=1, patch=2),
                    "gridhip_imager_mfdeconvolve_dev", SameT(vis), SameT(models), oi, 3, 0.25, 0.5, 7, 1, 2, st, handle=h)
    assert m is models and tensor_returned(oi, img, (T, N, N)) and tensor_returned(st, s, (3, 8))
    z, st = Zeros(T * N * N), Out(f64, 2 * 8)
    m, img, s = run(lambda: im.mfdeconvolve(vis, 2, out=images), "gridhip_imager_mfdeconvolve_dev", SameT(vis), z,
                    SameT(images), 2, 0.1, 0.0, 100, 0, 0, st, handle=h)
    assert img is images and tensor_returned(z.out, m, (T, N, N)) and tensor_returned(st, s, (2, 8))

    before = len(rec.calls)
    bad = [
        lambda: im.set_spectral(x, 0),
        lambda: im.set_spectral(x, 5),
        lambda: im.set_spectral(x[:-1], 2),
        lambda: im.set_spectral(x.numpy(), 2),
        lambda: im.mfs_cycle(vis[:-1]),
        lambda: im.mfs_cycle(vis.to(torch.complex64)),
        lambda: im.mfs_cycle(vis, models[:1]),
        lambda: im.mfs_cycle(vis, models.to(torch.float32)),
        lambda: im.mfs_cycle(vis, out=torch.zeros((3, N, N), dtype=torch.float64)),
        lambda: im.mfs_cycle(vis, vis_res=res[:-1]),
        lambda: im.mfclean(images[0]),
        lambda: im.mfclean(images.to(torch.float32)),
        lambda: im.mfclean(images, models=torch.zeros((T, N, N + 1), dtype=torch.float64)),
        lambda: im.mfdeconvolve(vis[:-1], 2),
        lambda: im.mfdeconvolve(vis, -1),
        lambda: im.mfdeconvolve(vis, 2, models=models.to(torch.float32)),
        lambda: im.mfdeconvolve(vis, 2, out=torch.zeros((T, N + 1, N + 1), dtype=torch.float64)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"
    assert im.nterms == T  # (a refused set_spectral leaves the terms as they were)
