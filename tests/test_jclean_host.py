"""Joint deconvolution (gridhip_jclean[_dev], Context.jclean, gridhip.joint_deconvolve), the checks that need no GPU: the
library, the header, the ctypes table, both bindings and the hpp carry the entry points; a NULL context is refused with
GRIDHIP_EINVAL; Context.jclean hands the ABI the right pointers, plane counts, scalar order and a 16-double stats buffer
(against the recording library of test_binding_marshalling.py) and refuses wrong dtypes, shapes, plane counts and weights
before any call; the numpy restatement the GPU tests compare with (tests/jclean_ref.py) is right on a case computed by
hand and, for one plane and the sum, is the Hogbom restatement with a stop level bit for bit; and the exact fixtures of
tests/jclean_cases.py are exact: the same runs in np.longdouble give the same numbers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clean_auto_ref
import clean_ref
import jclean_cases
import jclean_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Same  # noqa: F401
from test_clean_host import SameT, Zeros, rig, tensor_returned, torch_rig  # noqa: F401  (rig, torch_rig: fixtures)
from test_msclean_host import HostArr

NAMES = ["gridhip_jclean", "gridhip_jclean_dev"]
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
    assert _lib.SIGNATURES["gridhip_jclean"] == _lib.SIGNATURES["gridhip_jclean_dev"]
    assert len(_lib.SIGNATURES["gridhip_jclean"][1]) == 19
    assert _lib.load().gridhip_version() >= 310
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 310
    assert "joint deconvolution" in raw and int(re.search(r"#define GRIDHIP_JCLEAN_STATS (\d+)", raw).group(1)) == 16


def test_bindings_carry_the_entry_points():
    import gridhip
    assert callable(gridhip.Context.jclean) and callable(gridhip.joint_deconvolve) and "joint_deconvolve" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    assert "jcleanIO" in head and re.search(r"^jcleanIO ::", hs, flags=re.M) and "c_jclean c" in hs
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bjclean\s*\(", hpp) and "gridhip_jclean(" in hpp


def test_a_null_context_is_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_jclean.py::test_refusals); here: a NULL context is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    N, P = 4, 2
    psfs, res, mod = np.full(P * N * N, 1.0), np.full(P * N * N, 2.0), np.full(P * N * N, 3.0)
    stats, wts, noise = np.full(16, 7.0), np.full(P, 1.0), np.full(1, 5.0)
    p, r, m, s, n = (C.c_void_p(a.ctypes.data) for a in (psfs, res, mod, stats, noise))
    w = wts.ctypes.data_as(C.POINTER(C.c_double))
    for form in (lib.gridhip_jclean, lib.gridhip_jclean_dev):
        for sc in [(0.1, 0.0, 5, 0, 0), (0.0, 0.0, 5, 0, 0), (0.1, -1.0, 5, 0, 0), (0.1, 0.0, -1, 0, 0), (0.1, 0.0, 5, 2, 0)]:
            for planes, Q, metric in ((P, P, 0), (P, 1, 1), (0, 1, 0), (9, 9, 0), (P, 3, 0), (P, P, 2)):
                assert form(None, N, planes, Q, p, r, m, w, metric, *sc, None, 0.0, None, 0.0, s) == _lib.EINVAL
                assert form(None, N, planes, Q, p, r, m, None, metric, *sc, None, 3.0, n, 0.5, s) == _lib.EINVAL
    for a, val in ((psfs, 1.0), (res, 2.0), (mod, 3.0), (stats, 7.0), (wts, 1.0), (noise, 5.0)):
        assert np.all(a == val)


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
def hand_case():
    """N = 5, c = (2, 2), P = 2, one PSF: 1 at the centre, 0.5 at its four neighbours.  R_0 = 4 and R_1 = -2 at (3, 1),
    R_0 = 3 at (0, 4): sum with weights (1, 1): s = 2 at (3, 1) and 3 at (0, 4); sumsq: s = 20 at (3, 1) and 9 at (0, 4)."""
    psf = np.zeros((1, 5, 5))
    psf[0][2, 2] = 1.0
    psf[0][1, 2] = psf[0][3, 2] = psf[0][2, 1] = psf[0][2, 3] = 0.5
    res = np.zeros((2, 5, 5))
    res[0][3, 1], res[1][3, 1], res[0][0, 4] = 4.0, -2.0, 3.0
    return psf, res


def test_restatement_on_a_hand_computed_case():
    psf, res0 = hand_case()
    # sumsq: k = 16, s = 20, the gap (20 - 9) / 20; gain 0.5: f = (2, -1); the four neighbours lose f * 0.5
    res, models, trace = res0.copy(), np.zeros_like(res0), []
    st = jclean_ref.jclean(psf, res, models, None, 1, 0.5, 0.0, 1, trace=trace)
    assert trace == [(16, 11.0 / 20.0)]
    assert models[0][3, 1] == 2.0 and models[1][3, 1] == -1.0 and np.count_nonzero(models) == 2
    assert res[0][3, 1] == 2.0 and res[1][3, 1] == -1.0
    for y, x in ((2, 1), (4, 1), (3, 0), (3, 2)):
        assert res[0][y, x] == -1.0 and res[1][y, x] == 0.5
    assert res[0][0, 4] == 3.0 and np.count_nonzero(res[0]) == 6 and np.count_nonzero(res[1]) == 5
    # the final peak: (0, 4) with s = 9 against 4 + 1 = 5 at (3, 1); niter taken: reason 0; L = 0; s1 = 20
    assert np.array_equal(st, [1.0, 9.0, 4.0, 0.0, 0.0, 20.0, 0, 0, 2.0, -1.0, 0, 0, 0, 0, 0, 0])
    # the sum picks the other cell: s = 3 at (0, 4), whose PSF is clipped by two edges
    res, models = res0.copy(), np.zeros_like(res0)
    st = jclean_ref.jclean(psf, res, models, None, 0, 0.5, 0.0, 1)
    assert models[0][0, 4] == 1.5 and np.count_nonzero(models) == 1 and res[0][0, 4] == 1.5
    assert res[0][0, 3] == -0.75 and res[0][1, 4] == -0.75 and not res[1][0].any()
    assert np.array_equal(st[:6], [1.0, 2.0, 16.0, 0.0, 0.0, 3.0])
    # weights (1, 0): plane 1 does not steer - s = 4 at (3, 1) - and is still cleaned there
    res, models = res0.copy(), np.zeros_like(res0)
    st = jclean_ref.jclean(psf, res, models, [1.0, 0.0], 0, 0.5, 0.0, 1)
    assert models[0][3, 1] == 2.0 and models[1][3, 1] == -1.0 and st[5] == 4.0
    # stop levels: sumsq tests s <= T^2: threshold 4.5 is L = 20.25 > 20: reason 1 at once; 4.25: 18.0625, one component
    res, models = res0.copy(), np.zeros_like(res0)
    st = jclean_ref.jclean(psf, res, models, None, 1, 0.5, 4.5, 9)
    assert np.array_equal(st[:6], [0.0, 20.0, 16.0, 20.25, 1.0, 20.0]) and np.array_equal(res, res0)
    st = jclean_ref.jclean(psf, res, models, None, 1, 0.5, 4.25, 9)
    assert np.array_equal(st[:6], [1.0, 9.0, 4.0, 18.0625, 1.0, 20.0])
    # L = max(threshold^2, (nsigma * sigma)^2, peak_frac^2 * |s1|) = max(1, 2.25, 0.25 * 20)
    assert jclean_ref.stop_level(1.0, 3.0, 0.5, 0.5, 20.0, 1) == (5.0, False)
    assert jclean_ref.stop_level(1.0, 3.0, 0.5, 0.5, 20.0, 0) == (10.0, False)
    assert jclean_ref.stop_level(1.0, 0.0, math.nan, 0.0, 20.0, 1) == (1.0, False)
    assert jclean_ref.stop_level(1.0, 3.0, 0.5, 0.5, math.nan, 1) == (2.25, False)
    L, bad = jclean_ref.stop_level(1.0, 3.0, math.nan, 0.5, 20.0, 1)
    assert bad and math.isnan(L)
    # nothing selectable, NaN sigma, an all-zero mask
    st = jclean_ref.jclean(psf, np.full((2, 5, 5), np.nan), models, None, 1, 0.5, 0.0, 3)
    assert st[0] == 0 and math.isnan(st[1]) and st[2] == -1 and st[4] == 2 and math.isnan(st[5])
    res = res0.copy()
    st = jclean_ref.jclean(psf, res, models, None, 1, 0.5, 0.0, 3, nsigma=2.0, sigma=math.nan)
    assert st[0] == 0 and st[1] == 20.0 and st[2] == 16 and math.isnan(st[3]) and st[4] == 3 and np.array_equal(res, res0)
    st = jclean_ref.jclean(psf, res, models, None, 1, 0.5, 0.0, 3, mask=np.zeros((5, 5), dtype=np.uint8))
    assert st[0] == 0 and st[2] == -1 and st[4] == 2 and np.array_equal(res, res0)
    # a NaN in one plane hides its cell, under any weight
    res = res0.copy()
    res[1][0, 4] = np.nan
    for w in (None, [1.0, 0.0]):
        st = jclean_ref.jclean(psf, res.copy(), np.zeros_like(res), w, 0, 0.5, 0.0, 0)
        assert st[2] == 16


@pytest.mark.parametrize("N", [64, 63])
def test_one_plane_and_the_sum_is_the_hogbom_restatement_bit_for_bit(N):
    psf = clean_ref.make_psf(N, 3, fill=0.3)
    img, _ = clean_ref.make_sky(psf, 4, nsrc=6)
    mask = np.random.default_rng(5).random((N, N)) < 0.7
    for kw in (dict(), dict(mask=mask), dict(nsigma=3.0, sigma=0.02), dict(mask=mask, peak_frac=0.3, threshold=0.01),
               dict(nsigma=2.0, sigma=math.nan)):
        for border, patch in ((0, 0), (N // 8, 9)):
            r1, m1, t1 = img.copy(), np.zeros_like(img), []
            s1 = clean_auto_ref.clean(psf, r1, m1, 0.2, kw.get("threshold", 0.0), 40, border, patch,
                                      **{k: v for k, v in kw.items() if k != "threshold"}, trace=t1)
            r2, m2, t2 = img.copy()[None], np.zeros_like(img)[None], []
            s2 = jclean_ref.jclean(psf[None], r2, m2, jclean_ref.default_weights("sum", 1), 0, 0.2,
                                   kw.get("threshold", 0.0), 40, border, patch, trace=t2,
                                   **{k: v for k, v in kw.items() if k != "threshold"})
            assert np.array_equal(r1, r2[0]) and np.array_equal(m1, m2[0])
            # [iterations, peak, index, flux, T, reason, first peak] against [iterations, s, index, L, reason, s1, ..., flux_0]
            assert np.array_equal(s1[[0, 1, 2, 3, 4, 5, 6]], s2[[0, 1, 2, 8, 3, 4, 5]], equal_nan=True)
            assert [k for k, _ in t2] == [k for k, _, _ in t1][:len(t2)] and not s2[9:].any()


def test_the_gpu_test_inputs_meet_its_precondition():
    """tests/test_gpu_jclean.py's smallest cases, the restatement alone: the midway threshold stops the loop after some
    components and before many, 200 iterations take 200 components, and no gap between the two largest |s| is near 0"""
    N = 255
    for P, Q, metric in ((2, 2, 0), (4, 1, 1)):
        psfs, img = jclean_ref.make_psfs(N, Q), jclean_ref.make_sky(N, P, Q)
        w = jclean_ref.default_weights(("sum", "sumsq")[metric], P)
        mid = jclean_ref.midway_threshold(psfs, img, w, metric)
        for threshold, niter in ((0.0, 200), (mid, 200)):
            trace = []
            st = jclean_ref.jclean(psfs, img.copy(), np.zeros_like(img), w, metric, 0.2, threshold, niter, trace=trace)
            assert (0 < st[0] < niter and st[4] == 1) if threshold > 0.0 else (st[0] == niter and st[4] == 0), st
            assert len(trace) == st[0] and min(g for _, g in trace) > 1e-8


# ---- the exact fixtures are exact ------------------------------------------------------------------------------------------
FIXTURES = jclean_cases.all_fixtures()


def test_the_fixture_names_are_unique_and_cover_the_placements():
    names = [f.name for f in FIXTURES]
    assert len(set(names)) == len(names)
    assert {f.N for f in FIXTURES} >= {1, 2, 3, 4, 5, 17, 129} and {f.P for f in FIXTURES} >= {2, 3, 4, 8}
    assert any(f.N % 2 and f.P >= 2 and f.Q == f.P for f in FIXTURES) and any(f.Q == 1 and f.P > 1 for f in FIXTURES)


@pytest.mark.parametrize("f", FIXTURES, ids=lambda f: f.name)
def test_an_exact_fixture_is_exact(f):
    """the run in np.longdouble gives the same numbers: no operation of the fp64 run rounded"""
    trace = []
    m, r, s = jclean_cases.reference(f, trace=trace)
    if np.finfo(np.longdouble).nmant > 52:
        ml, rl, sl = jclean_cases.reference(f, np.longdouble)
        assert np.array_equal(ml.astype(f64), m) and np.array_equal(ml, m.astype(np.longdouble))
        assert np.array_equal(rl, r.astype(np.longdouble), equal_nan=True)
        assert np.array_equal(sl, s.astype(np.longdouble), equal_nan=True)
    # what the fixture is for
    if f.name.startswith("tie-"):
        assert trace[0][1] == 0.0, "the first pick is a tie"
        assert trace[0][0] == min(y * f.N + x for _, y, x, _ in f.cells), "the lowest flat index wins"
    elif f.name.startswith("size-"):
        assert s[0] == f.niter and s[4] == 0 and m.all(axis=0).any()
    elif f.name.startswith(("all-nan", "one-plane-nan", "zero-mask")):
        assert s[0] == 0 and s[2] == -1 and s[4] == 2 and not m.any()
    elif f.name.startswith("nan-sigma"):
        assert s[0] == 0 and s[4] == 3 and math.isnan(s[3]) and not m.any()
    elif f.name.startswith(("nan-in-plane-2", "nan-under-weight-0", "masked-peak")):
        assert not m[:, 5, 7].any() and m[0][9, 3] != 0.0 and s[0] == f.niter
    elif f.name.startswith("stop-level"):
        assert 0 < s[0] < f.niter and s[4] == 1 and s[3] == (10.0, 100.0)[f.metric] and abs(s[1]) <= s[3]
    elif f.name.startswith("weights-1000"):
        # plane 0's own sequence: the Hogbom restatement of plane 0 alone finds the same cells and the same plane 0
        psf, res = jclean_cases.exact_psfs(f.N, f.Q)[0], jclean_cases.residuals_of(f)[0]
        m0 = np.zeros_like(res)
        clean_auto_ref.clean(np.array(psf), res, m0, f.gain, 0.0, f.niter, f.border, f.patch)
        assert np.array_equal(m0, m[0]) and np.array_equal(res, r[0])
        for p in range(1, f.P):
            assert np.array_equal(np.flatnonzero(m[p]), np.flatnonzero(m[0]))
        assert abs(r[1][8, 8]) == 40.0  # the largest value of all, in a plane of weight 0, was never a peak
    elif f.name.startswith("weights-0201"):
        assert m[1][8, 8] != 0.0 and m[0][8, 8] != 0.0 and not m[:, 4, 4].any()


# ---- what the Python method hands to the ABI ------------------------------------------------------------------------------
def test_context_jclean_host_form(rig):  # noqa: F811
    ctx, rec, run = rig
    N, P = 6, 4
    images = np.arange(P * N * N, dtype=f64).reshape(P, N, N)
    psf32 = np.arange(N * N, dtype=np.float32).reshape(N, N)  # one PSF, float32: converted, Q = 1
    models = np.ones((P, N, N))
    mask = np.ones((N, N), dtype=bool)
    st = Out(f64, 16)
    m, r, s = run(lambda: ctx.jclean(images, psf32, "sum", [1, 0, 0, 2], gain=0.25, threshold=0.5, niter=7, border=1, patch=2,
                                     models=models, mask=mask, nsigma=3.0, noise=0.125, peak_frac=0.5),
                  "gridhip_jclean", N, P, 1, Arr(psf32, f64), Same(images), Same(models), HostArr([1, 0, 0, 2]), 0, 0.25, 0.5,
                  7, 1, 2, Arr(np.ones(N * N), np.uint8), 3.0, Arr([0.125], f64), 0.5, st)
    assert m is models and r is images and st.returned(s, (16,))
    # defaults: sumsq, weights 1 each, no mask, no noise; a PSF per plane in the right form goes by its own address
    psfs = np.zeros((P, N, N))
    z, st = Zeros(P * N * N), Out(f64, 16)
    m, r, s = run(lambda: ctx.jclean(images, psfs), "gridhip_jclean", N, P, P, Same(psfs), Same(images), z,
                  HostArr([1.0] * P), 1, 0.1, 0.0, 100, 0, 0, None, 0.0, None, 0.0, st)
    assert r is images and z.out.returned(m, (P, N, N)) and st.returned(s, (16,))
    # the sum's default weights are 1 / P: the mean image; a [1, N, N] stack is one PSF
    one = np.zeros((1, N, N))
    run(lambda: ctx.jclean(images[:3].copy(), one, "sum"), "gridhip_jclean", N, 3, 1, Same(one), Arr(images[:3], f64),
        Zeros(3 * N * N), HostArr([1.0 / 3] * 3), 0, 0.1, 0.0, 100, 0, 0, None, 0.0, None, 0.0, Out(f64, 16))
    before = len(rec.calls)
    bad = [
        lambda: ctx.jclean(images.astype(np.float32), psfs),               # updated in place: no conversion
        lambda: ctx.jclean(images[0], psfs[0]),                            # not a stack
        lambda: ctx.jclean(np.zeros((9, N, N)), np.zeros((9, N, N))),      # P = 9
        lambda: ctx.jclean(np.zeros((0, N, N)), np.zeros((0, N, N))),      # P = 0
        lambda: ctx.jclean(np.zeros((P, N, N + 1)), psfs),                 # not square
        lambda: ctx.jclean(images, psfs[:2]),                              # two PSFs for four planes
        lambda: ctx.jclean(images, np.zeros((N + 1, N + 1))),
        lambda: ctx.jclean(images, psfs, models=np.zeros((P, N, N), dtype=np.float32)),
        lambda: ctx.jclean(images, psfs, models=np.zeros((1, N, N))),
        lambda: ctx.jclean(np.zeros((P, N, 2 * N))[:, :, ::2], psfs),      # not contiguous
        lambda: ctx.jclean(images, psfs, weights=[1, 1, -1, 1]),           # a negative weight
        lambda: ctx.jclean(images, psfs, weights=[0, 0, 0, 0]),
        lambda: ctx.jclean(images, psfs, weights=[1, 1, float("nan"), 1]),
        lambda: ctx.jclean(images, psfs, weights=[1, 1, 1]),
        lambda: ctx.jclean(images, psfs, metric="max"),
        lambda: ctx.jclean(images, psfs, mask=np.ones((N, N))),            # a float mask
        lambda: ctx.jclean(images, psfs, mask=np.ones((P, N, N), dtype=bool)),  # one mask, not one per plane
        lambda: ctx.jclean(images, psfs, nsigma=3.0),                      # no noise
        lambda: ctx.jclean(images, psfs, peak_frac=1.0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"


def test_context_jclean_device_form(torch_rig):  # noqa: F811
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, P = 6, 3
    images = torch.arange(P * N * N, dtype=torch.float64).reshape(P, N, N)
    psfs32 = torch.arange(P * N * N, dtype=torch.float32).reshape(P, N, N)
    models = torch.ones((P, N, N), dtype=torch.float64)
    noise = torch.full((1,), 0.25, dtype=torch.float64)
    st = Out(f64, 16)
    m, r, s = run(lambda: ctx.jclean(images, psfs32, "sumsq", torch.tensor([1.0, 2.0, 0.0]), 0.25, 0.5, 7, 1, 2, models, None,
                                     2.0, noise, 0.0),
                  "gridhip_jclean_dev", N, P, P, Arr(psfs32.numpy(), f64), SameT(images), SameT(models), HostArr([1, 2, 0]), 1,
                  0.25, 0.5, 7, 1, 2, None, 2.0, SameT(noise), 0.0, st)
    assert m is models and r is images and tensor_returned(st, s, (16,)) and bound == [ctx]
    for call in (lambda: ctx.jclean(images.to(torch.float32), psfs32), lambda: ctx.jclean(images, psfs32[:2]),
                 lambda: ctx.jclean(images, psfs32, models=np.zeros((P, N, N))),
                 lambda: ctx.jclean(images, psfs32, weights=[1.0, -2.0, 0.0])):
        with pytest.raises(ValueError):
            call()
    assert rec.calls.count("gridhip_jclean_dev") == 1
