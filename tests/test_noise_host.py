"""Image statistics, clean masks and noise-based stop levels (gridhip_image_stats*, gridhip_*clean_auto*,
gridhip_imager_*deconvolve_auto_dev), the checks that need no GPU: the library, the header, the ctypes table and the
bindings carry every new name; a NULL handle is refused with nothing touched; the Python methods hand the ABI the right
pointers, order and stats sizes (against a recording library) and still take today's entry points when the new keywords
are left alone; wrong masks are refused before any call; and the numpy restatements the GPU tests compare with
(tests/noise_ref.py, tests/clean_auto_ref.py) are right on cases computed by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clean_auto_ref
import clean_ref
import noise_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Same
from test_clean_host import SameT, Zeros, rig, tensor_returned, torch_rig  # noqa: F401  (fixtures)

NAMES = ["gridhip_image_stats", "gridhip_image_stats_dev", "gridhip_imager_image_stats_dev", "gridhip_clean_auto",
         "gridhip_clean_auto_dev", "gridhip_msclean_auto", "gridhip_msclean_auto_dev", "gridhip_imager_clean_auto_dev",
         "gridhip_imager_msclean_auto_dev", "gridhip_imager_deconvolve_auto_dev", "gridhip_imager_msdeconvolve_auto_dev"]
f64 = np.float64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_names():
    from gridhip import _lib
    text = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    for host_form in ("gridhip_image_stats", "gridhip_clean_auto", "gridhip_msclean_auto"):
        assert _lib.SIGNATURES[host_form] == _lib.SIGNATURES[host_form + "_dev"]
    assert "mask" in text and _lib.load().gridhip_version() >= 190


def test_bindings_carry_the_names():
    import gridhip
    for cls in (gridhip.Context, gridhip.Imager):
        assert callable(cls.image_stats)
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("imageStatsIO", "cleanAutoIO", "imagerDeconvolveAutoIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    for name in ("gridhip_image_stats", "gridhip_clean_auto", "gridhip_msclean_auto"):
        assert name + "(" in hpp, name


def test_null_handles_are_refused_and_nothing_is_touched():
    from gridhip import _lib
    lib = _lib.load()
    N = 4
    arrs = [np.full(N * N, v) for v in (1.0, 2.0, 3.0)]
    mask = np.full(N * N, 5, dtype=np.uint8)
    stats, noise = np.full(16, 7.0), np.full(1, 9.0)
    p, r, m = (C.c_void_p(a.ctypes.data) for a in arrs)
    k, s, z = C.c_void_p(mask.ctypes.data), C.c_void_p(stats.ctypes.data), C.c_void_p(noise.ctypes.data)
    sc = (C.c_double * 2)(0.0, 2.0)
    cl = (0.1, 0.0, 5, 0, 0)
    for auto in ((k, 3.0, z, 0.1), (None, 0.0, None, 0.0), (k, -1.0, z, 0.1), (k, 3.0, None, 0.1), (k, 3.0, z, 1.0),
                 (k, float("nan"), z, float("nan"))):
        assert lib.gridhip_clean_auto(None, N, p, r, m, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_clean_auto_dev(None, N, p, r, m, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_msclean_auto(None, N, p, r, m, 2, sc, sc, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_msclean_auto_dev(None, N, p, r, m, 2, sc, sc, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_imager_clean_auto_dev(None, r, m, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_imager_msclean_auto_dev(None, r, m, 2, sc, sc, *cl, *auto, s) == _lib.EINVAL
        assert lib.gridhip_imager_deconvolve_auto_dev(None, p, m, r, 2, *cl, auto[0], auto[1], auto[3], s, s) == _lib.EINVAL
        assert lib.gridhip_imager_msdeconvolve_auto_dev(None, p, m, r, 2, 2, sc, sc, *cl, auto[0], auto[1], auto[3], s,
                                                        None) == _lib.EINVAL
    for n_, img, mk, border in ((N, r, k, 0), (N, r, None, 0), (0, r, k, 0), (N, None, k, 0), (N, r, k, 2), (N, r, k, -1)):
        assert lib.gridhip_image_stats(None, n_, img, mk, border, s) == _lib.EINVAL
        assert lib.gridhip_image_stats_dev(None, n_, img, mk, border, s) == _lib.EINVAL
        assert lib.gridhip_imager_image_stats_dev(None, img, mk, border, s) == _lib.EINVAL
    for a, v in zip(arrs, (1.0, 2.0, 3.0)):
        assert np.all(a == v)
    assert np.all(mask == 5) and np.all(stats == 7.0) and noise[0] == 9.0


# ---- the restatements on cases computed by hand ---------------------------------------------------------------------------
def test_image_stats_restatement_on_a_hand_computed_case():
    """3 x 3: the values 1 .. 9 shuffled.  n = 9, rank 4: median 5; d = 4 3 2 1 0 1 2 3 4, sorted 0 1 1 2 2 3 3 4 4, rank
    4: MAD 2.  With a NaN and an Inf: they are skipped and counted.  With a mask leaving 4, 8: n = 2, rank 0: the LOWER
    median 4, d = 0, 4, MAD 0.  -0.0 sorts before +0.0."""
    img = np.array([[7.0, 2.0, 9.0], [4.0, 5.0, 1.0], [8.0, 3.0, 6.0]])
    assert np.array_equal(noise_ref.image_stats(img), [9.0, 5.0, 2.0, 1.4826 * 2.0, 1.0, 9.0, 0.0, 0.0])
    bad = img.copy()
    bad[0, 0], bad[2, 2] = np.nan, np.inf  # 7 and 6 leave: 1 2 3 4 5 8 9, rank 3: 4; d = 3 2 1 0 1 4 5 -> 0 1 1 2 3 4 5: 2
    assert np.array_equal(noise_ref.image_stats(bad), [7.0, 4.0, 2.0, 1.4826 * 2.0, 1.0, 9.0, 2.0, 0.0])
    mask = np.zeros((3, 3), dtype=np.uint8)
    mask[1, 0], mask[2, 0] = 1, 200
    assert np.array_equal(noise_ref.image_stats(img, mask), [2.0, 4.0, 0.0, 0.0, 4.0, 8.0, 0.0, 0.0])
    st = noise_ref.image_stats(img, border=1)  # the centre cell alone
    assert np.array_equal(st, [1.0, 5.0, 0.0, 0.0, 5.0, 5.0, 0.0, 0.0])
    st = noise_ref.image_stats(img, np.zeros((3, 3), dtype=bool))
    assert st[0] == 0 and np.isnan(st[1:6]).all() and st[6] == 0
    z = np.array([[0.0, -0.0], [-0.0, 0.0]])
    st = noise_ref.image_stats(z)  # keys: -0 -0 +0 +0, rank 1: -0.0; min -0.0, max +0.0
    assert np.signbit(st[1]) and np.signbit(st[4]) and not np.signbit(st[5]) and st[2] == 0.0
    k = noise_ref.keys(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf]))
    assert np.all(k[1:] > k[:-1]) and np.array_equal(noise_ref.values(k)[[1, 5]], [-1.0, 1.0])


def hand_case():
    psf = np.zeros((5, 5))
    psf[2, 2] = 1.0
    psf[1, 2] = psf[3, 2] = psf[2, 1] = psf[2, 3] = 0.5
    res = np.zeros((5, 5))
    res[0, 4], res[3, 1] = -2.0, 2.0
    return psf, res


def test_the_mask_moves_the_first_component():
    """clean_ref's hand case: -2 at (0, 4) and +2 at (3, 1); the lower index goes first.  A mask without (0, 4) makes
    (3, 1) the first and only component: the PSF is still subtracted over masked-out cells, and the final peak is the
    peak under the mask - the untouched -2 at (0, 4) is not reported."""
    psf, res = hand_case()
    model = np.zeros((5, 5))
    mask = np.ones((5, 5), dtype=np.uint8)
    mask[0, 4] = 0
    st = clean_auto_ref.clean(psf, res, model, 0.5, 0.0, 1, mask=mask)
    want = np.zeros((5, 5))
    want[0, 4], want[3, 1], want[2, 1], want[4, 1], want[3, 0], want[3, 2] = -2.0, 1.0, -0.5, -0.5, -0.5, -0.5
    assert np.array_equal(res, want) and model[3, 1] == 1.0 and np.count_nonzero(model) == 1
    assert np.array_equal(st, [1.0, 1.0, 16.0, 1.0, 0.0, 0.0, 2.0, 0.0])  # reason 0: niter; p1 = +2
    # neutral arguments: clean_ref's bits and stats
    psf, a = hand_case()
    b, ma, mb = a.copy(), np.zeros((5, 5)), np.zeros((5, 5))
    sa, sb = clean_auto_ref.clean(psf, a, ma, 0.5, 0.0, 2), clean_ref.clean(psf, b, mb, 0.5, 0.0, 2)
    assert np.array_equal(a, b) and np.array_equal(ma, mb) and np.array_equal(sa[:4], sb) and sa[5] == 0
    # an empty mask: nothing selectable, nothing touched; a NaN sigma: reason 3, nothing touched
    psf, a = hand_case()
    st = clean_auto_ref.clean(psf, a, ma, 0.5, 0.0, 2, mask=np.zeros((5, 5), dtype=bool))
    assert st[0] == 0 and np.isnan(st[1]) and st[2] == -1 and st[5] == 2 and np.array_equal(a, hand_case()[1])
    st = clean_auto_ref.clean(psf, a, ma, 0.5, 0.0, 2, nsigma=3.0, sigma=np.nan)
    assert st[0] == 0 and st[5] == 3 and np.isnan(st[4]) and np.array_equal(a, hand_case()[1])


def test_peak_frac_stops_the_loop_at_a_known_iteration():
    """One source of 8 at the centre, a delta PSF, gain 0.5: the peaks are 8, 4, 2, 1 ...  peak_frac 0.2: T = 1.6, so the
    components at 8, 4 and 2 are taken and the loop stops at the peak 1 (reason 1) after 3 iterations.  nsigma 3 with
    sigma 1 binds instead: T = 3, two components, the final peak 2."""
    psf = np.zeros((5, 5))
    psf[2, 2] = 1.0
    res, model = np.zeros((5, 5)), np.zeros((5, 5))
    res[2, 2] = 8.0
    st = clean_auto_ref.clean(psf, res, model, 0.5, 0.0, 50, peak_frac=0.2)
    assert np.array_equal(st, [3.0, 1.0, 12.0, 7.0, 0.2 * 8.0, 1.0, 8.0, 0.0]) and model[2, 2] == 7.0
    res, model = np.zeros((5, 5)), np.zeros((5, 5))
    res[2, 2] = 8.0
    st = clean_auto_ref.clean(psf, res, model, 0.5, 0.5, 50, nsigma=3.0, sigma=1.0, peak_frac=0.2)
    assert np.array_equal(st, [2.0, 2.0, 12.0, 6.0, 3.0, 1.0, 8.0, 0.0])
    res, model = np.zeros((5, 5)), np.zeros((5, 5))
    res[2, 2] = 8.0
    st = clean_auto_ref.msclean(psf, res, model, [0.0], [1.0], 0.5, 0.0, 50, peak_frac=0.2)
    assert np.array_equal(st[[0, 1, 2, 3, 4, 6]], [3.0, 1.0, 12.0, 0.0, 7.0, 3.0])
    assert np.array_equal(st[12:], [1.6, 1.0, 8.0, 0.0]) and model[2, 2] == 7.0
    a = 1.0 + 2.0 ** -30  # a * a = 1 + 2^-29 + 2^-60: the last term is lost when the product is rounded first
    assert clean_auto_ref.fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60 and a * a - 1.0 == 2.0 ** -29


# ---- what the Python methods hand to the ABI ------------------------------------------------------------------------------
def test_context_image_stats_and_clean_host_forms(rig):
    ctx, rec, run = rig
    N = 6
    image = np.arange(N * N, dtype=f64).reshape(N, N)
    psf = np.zeros((N, N))
    model = np.ones((N, N))
    mask8 = (np.arange(N * N).reshape(N, N) % 3).astype(np.uint8)
    maskb = mask8 != 0
    st = Out(f64, 8)
    s = run(lambda: ctx.image_stats(image, mask8, border=1), "gridhip_image_stats", N, Same(image), Same(mask8), 1, st)
    assert st.returned(s, (8,))
    st = Out(f64, 8)
    s = run(lambda: ctx.image_stats(image.astype(np.float32)), "gridhip_image_stats", N, Arr(image, f64), None, 0, st)
    assert st.returned(s, (8,))
    # a bool mask goes as its own bytes; sigma as a number becomes one double
    st = Out(f64, 8)
    m, r, s = run(lambda: ctx.clean(image, psf, 0.25, 0.5, 7, 1, 2, model, mask=maskb, nsigma=3.0, noise=0.125, peak_frac=0.1),
                  "gridhip_clean_auto", N, Same(psf), Same(image), Same(model), 0.25, 0.5, 7, 1, 2,
                  Same(maskb), 3.0, Arr([0.125], f64), 0.1, st)
    assert m is model and r is image and st.returned(s, (8,))
    # one element of a stats array goes by its own address; no mask is NULL
    stats = np.arange(8, dtype=f64)
    st = Out(f64, 8)
    run(lambda: ctx.clean(image, psf, model=model, nsigma=2.0, noise=stats[3:4]), "gridhip_clean_auto", N, Same(psf),
        Same(image), Same(model), 0.1, 0.0, 100, 0, 0, None, 2.0, Same(stats, 24), 0.0, st)
    st = Out(f64, 16)
    m, r, s = run(lambda: ctx.msclean(image, psf, [0.0, 2.0], model=model, mask=mask8, peak_frac=0.5), "gridhip_msclean_auto",
                  N, Same(psf), Same(image), Same(model), 2, ScalesArr([0.0, 2.0]), ScalesArr([1.0, 0.4]),
                  0.1, 0.0, 100, 0, 0, Same(mask8), 0.0, None, 0.5, st)
    assert st.returned(s, (16,))
    # the keywords left alone: today's entry points and today's stats
    st = Out(f64, 4)
    m, r, s = run(lambda: ctx.clean(image, psf, model=model), "gridhip_clean", N, Same(psf), Same(image), Same(model),
                  0.1, 0.0, 100, 0, 0, st)
    assert st.returned(s, (4,))
    st = Out(f64, 12)
    m, r, s = run(lambda: ctx.msclean(image, psf, [0.0, 2.0], model=model), "gridhip_msclean", N, Same(psf), Same(image),
                  Same(model), 2, ScalesArr([0.0, 2.0]), ScalesArr([1.0, 0.4]), 0.1, 0.0, 100, 0, 0, st)
    assert st.returned(s, (12,))


class ScalesArr:
    """a POINTER(c_double) argument addressing these values"""

    def __init__(self, values):
        self.want = np.array(values, dtype=f64)

    def check(self, arg, where):
        got = np.array([arg[i] for i in range(self.want.size)])
        assert np.allclose(got, self.want, rtol=1e-15), f"{where}: {got} != {self.want}"


def test_wrong_masks_and_levels_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    N = 6
    image, psf = np.zeros((N, N)), np.zeros((N, N))
    ok = np.ones((N, N), dtype=np.uint8)
    bad = [
        lambda: ctx.image_stats(image, ok.astype(np.int32)),
        lambda: ctx.image_stats(image, ok.astype(np.float64)),
        lambda: ctx.image_stats(image, ok[:, :5]),
        lambda: ctx.image_stats(image, ok.ravel()),
        lambda: ctx.image_stats(image, [[1] * N] * N),
        lambda: ctx.image_stats(np.zeros((N, N + 1))),
        lambda: ctx.clean(image, psf, mask=ok.astype(np.int8)),
        lambda: ctx.clean(image, psf, mask=np.ones((N + 1, N + 1), dtype=bool)),
        lambda: ctx.clean(image, psf, nsigma=3.0),                       # no noise
        lambda: ctx.clean(image, psf, nsigma=-1.0, noise=1.0),
        lambda: ctx.clean(image, psf, nsigma=float("inf"), noise=1.0),
        lambda: ctx.clean(image, psf, peak_frac=1.0),
        lambda: ctx.clean(image, psf, peak_frac=float("nan")),
        lambda: ctx.clean(image, psf, nsigma=1.0, noise=np.zeros(2)),
        lambda: ctx.clean(image, psf, nsigma=1.0, noise=np.zeros(1, dtype=np.float32)),
        lambda: ctx.msclean(image, psf, [0.0], mask=ok.astype(np.uint16)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert rec.calls == [], f"refusal {k} came after {rec.calls}"


def test_imager_forms(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, n, h = im.N, im.n, im._h
    image = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    model = torch.ones((N, N), dtype=torch.float64)
    vis = torch.arange(n, dtype=torch.float64).to(torch.complex128)
    mask = torch.ones((N, N), dtype=torch.bool)
    mask8 = torch.ones((N, N), dtype=torch.uint8)
    sig = torch.arange(8, dtype=torch.float64)
    st = Out(f64, 8)
    s = run(lambda: im.image_stats(image, mask, 1), "gridhip_imager_image_stats_dev", SameT(image), SameT(mask), 1, st,
            handle=h)
    assert tensor_returned(st, s, (8,)) and bound == [ctx]
    st = Out(f64, 8)
    s = run(lambda: ctx.image_stats(image), "gridhip_image_stats_dev", N, SameT(image), None, 0, st)
    assert tensor_returned(st, s, (8,))
    st = Out(f64, 8)
    m, r, s = run(lambda: im.clean(image, model, 0.25, 0.5, 7, 1, 2, mask=mask8, nsigma=3.0, noise=sig[3:4]),
                  "gridhip_imager_clean_auto_dev", SameT(image), SameT(model), 0.25, 0.5, 7, 1, 2, SameT(mask8), 3.0,
                  SameT(sig[3:4]), 0.0, st, handle=h)
    assert m is model and r is image and tensor_returned(st, s, (8,))
    st = Out(f64, 16)
    m, r, s = run(lambda: im.msclean(image, [0.0, 2.0], model=model, peak_frac=0.25), "gridhip_imager_msclean_auto_dev",
                  SameT(image), SameT(model), 2, ScalesArr([0.0, 2.0]), ScalesArr([1.0, 0.4]), 0.1, 0.0, 100, 0, 0, None,
                  0.0, None, 0.25, st, handle=h)
    assert tensor_returned(st, s, (16,))
    # the loop: stats and istats, one row per major cycle
    st, ist, oi = Out(f64, 3 * 8), Out(f64, 3 * 8), Out(f64, N * N)
    out = run(lambda: im.deconvolve(vis, 3, model=model, gain=0.25, threshold=0.5, niter=7, border=1, patch=2, mask=mask,
                                    nsigma=3.0, peak_frac=0.1),
              "gridhip_imager_deconvolve_auto_dev", SameT(vis), SameT(model), oi, 3, 0.25, 0.5, 7, 1, 2, SameT(mask), 3.0, 0.1,
              Both(st), Both(ist), handle=h)
    assert len(out) == 4 and out[0] is model and tuple(out[2].shape) == (3, 8) and tuple(out[3].shape) == (3, 8)
    assert out[2].data_ptr() != out[3].data_ptr()
    out = run(lambda: im.deconvolve(vis, 2, model=model, scales=[0.0, 2.0], nsigma=3.0),
              "gridhip_imager_msdeconvolve_auto_dev", SameT(vis), SameT(model), Out(f64, N * N), 2, 2, ScalesArr([0.0, 2.0]),
              ScalesArr([1.0, 0.4]), 0.1, 0.0, 100, 0, 0, None, 3.0, 0.0, Out(f64, 2 * 16), Out(f64, 2 * 8), handle=h)
    assert tuple(out[2].shape) == (2, 16) and tuple(out[3].shape) == (2, 8)
    # the keywords left alone: today's entry points
    st = Out(f64, 4)
    run(lambda: im.clean(image, model), "gridhip_imager_clean_dev", SameT(image), SameT(model), 0.1, 0.0, 100, 0, 0, st,
        handle=h)
    run(lambda: im.deconvolve(vis, 2, model=model), "gridhip_imager_deconvolve_dev", SameT(vis), SameT(model),
        Out(f64, N * N), 2, 0.1, 0.0, 100, 0, 0, Out(f64, 8), handle=h)
    before = len(rec.calls)
    bad = [
        lambda: im.image_stats(image, mask.to(torch.int32)),
        lambda: im.image_stats(image, mask[:5, :5].contiguous()),
        lambda: im.image_stats(image, np.ones((N, N), dtype=bool)),
        lambda: im.image_stats(image.to(torch.float32)),
        lambda: im.clean(image, model, mask=mask.to(torch.float64)),
        lambda: im.clean(image, model, nsigma=3.0),
        lambda: im.deconvolve(vis, 2, mask=mask.to(torch.int64)),
        lambda: im.deconvolve(vis, 2, peak_frac=1.5),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"


class Both:
    """an output the recorder fills"""

    def __init__(self, out):
        self.out = out

    def check(self, arg, where):
        self.out.check(arg, where)
