"""Deconvolution (gridhip_clean*, gridhip_imager_clean_dev, gridhip_imager_deconvolve_dev), the checks that need no GPU:
the library, the header, the ctypes table and both bindings carry the four entry points; a NULL context or imager is
refused with GRIDHIP_EINVAL whatever else is passed; Context.clean, Imager.clean and Imager.deconvolve hand the ABI the
right pointers, shapes, scalar order and stats buffer (against a recording library, as test_binding_marshalling.py does)
and refuse wrong dtypes and shapes before any call; and the numpy restatement the GPU tests compare with
(tests/clean_ref.py) is right on a case computed by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clean_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same, address

NAMES = ["gridhip_clean", "gridhip_clean_dev", "gridhip_imager_clean_dev", "gridhip_imager_deconvolve_dev"]
f64 = np.float64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_clean():
    from gridhip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gridhip.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_clean"] == _lib.SIGNATURES["gridhip_clean_dev"]
    assert _lib.load().gridhip_version() >= 160


def test_bindings_carry_clean():
    import gridhip
    assert callable(gridhip.Context.clean) and callable(gridhip.Imager.clean) and callable(gridhip.Imager.deconvolve)
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("cleanIO", "imagerCleanIO", "imagerDeconvolveIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bclean\s*\(", hpp) and "gridhip_clean" in hpp


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_clean.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    N = 4
    arrs = [np.full(N * N, v) for v in (1.0, 2.0, 3.0)]
    stats = np.full(12, 7.0)
    p, r, m = (C.c_void_p(a.ctypes.data) for a in arrs)
    s = C.c_void_p(stats.ctypes.data)
    good = (0.1, 0.0, 5, 0, 0)
    bad = [(0.0, 0.0, 5, 0, 0), (1.5, 0.0, 5, 0, 0), (float("nan"), 0.0, 5, 0, 0), (0.1, -1.0, 5, 0, 0),
           (0.1, 0.0, -1, 0, 0), (0.1, 0.0, 5, -1, 0), (0.1, 0.0, 5, 2, 0), (0.1, 0.0, 5, 0, -1)]
    for sc in [good] + bad:
        assert lib.gridhip_clean(None, N, p, r, m, *sc, s) == _lib.EINVAL
        assert lib.gridhip_clean_dev(None, N, p, r, m, *sc, s) == _lib.EINVAL
        assert lib.gridhip_imager_clean_dev(None, r, m, *sc, s) == _lib.EINVAL
        assert lib.gridhip_imager_deconvolve_dev(None, p, m, r, 2, *sc, s) == _lib.EINVAL
    for n_, pp, rr, mm in ((0, p, r, m), (N, None, r, m), (N, p, None, m), (N, p, r, None), (N, p, r, r), (N, p, p, m)):
        assert lib.gridhip_clean(None, n_, pp, rr, mm, *good, None) == _lib.EINVAL
    for a, v in zip(arrs, (1.0, 2.0, 3.0)):
        assert np.all(a == v)
    assert np.all(stats == 7.0)


# ---- the numpy restatement on a case computed by hand --------------------------------------------------------------------
def test_restatement_on_a_hand_computed_case():
    """N = 5, c = (2, 2); PSF: 1 at the centre, 0.5 at its four neighbours.  The residual holds -2 at (0, 4), a corner,
    and +2 at (3, 1): equal magnitudes, so the lower flat index (4) goes first, and its PSF is clipped by two edges.
    gain 0.5: f = -1 at (0, 4), then f = +1 at (3, 1)."""
    psf = np.zeros((5, 5))
    psf[2, 2] = 1.0
    psf[1, 2] = psf[3, 2] = psf[2, 1] = psf[2, 3] = 0.5
    res = np.zeros((5, 5))
    res[0, 4], res[3, 1] = -2.0, 2.0
    model = np.zeros((5, 5))
    trace = []
    stats = clean_ref.clean(psf, res, model, 0.5, 0.0, 1, trace=trace)
    want = np.zeros((5, 5))
    want[0, 4], want[0, 3], want[1, 4], want[3, 1] = -1.0, 0.5, 0.5, 2.0  # (0, 5) and (-1, 4) are outside: clipped
    assert np.array_equal(res, want) and trace == [(4, 0.0)]
    assert model[0, 4] == -1.0 and np.count_nonzero(model) == 1
    assert np.array_equal(stats, [1.0, 2.0, 16.0, -1.0])
    stats = clean_ref.clean(psf, res, model, 0.5, 0.0, 1)
    want[3, 1], want[2, 1], want[4, 1], want[3, 0], want[3, 2] = 1.0, -0.5, -0.5, -0.5, -0.5
    assert np.array_equal(res, want)
    assert model[3, 1] == 1.0 and model[0, 4] == -1.0 and np.count_nonzero(model) == 2
    assert np.array_equal(stats, [1.0, -1.0, 4.0, 1.0])  # the tie of the final residual, again to the lower index
    # the same two components in one call; then: the threshold is tested before anything is subtracted, niter = 0
    # reports the peak, the border hides the corner, the patch cuts the PSF, a NaN is never selected
    res2, model2 = np.zeros((5, 5)), np.zeros((5, 5))
    res2[0, 4], res2[3, 1] = -2.0, 2.0
    assert np.array_equal(clean_ref.clean(psf, res2, model2, 0.5, 0.0, 2), [2.0, -1.0, 4.0, 0.0])
    assert np.array_equal(res2, want) and np.array_equal(model2, model)
    before = res2.copy()
    assert np.array_equal(clean_ref.clean(psf, res2, model2, 0.5, 1.0, 9), [0.0, -1.0, 4.0, 0.0])
    assert np.array_equal(clean_ref.clean(psf, res2, model2, 0.5, 0.0, 0), [0.0, -1.0, 4.0, 0.0])
    assert np.array_equal(res2, before) and np.array_equal(model2, model)
    assert np.array_equal(clean_ref.clean(psf, res2, model2, 0.5, 0.0, 0, border=1), [0.0, 1.0, 16.0, 0.0])
    res3, model3 = np.zeros((5, 5)), np.zeros((5, 5))
    res3[2, 2] = 4.0
    wide = np.full((5, 5), 0.25)
    wide[2, 2] = 1.0
    clean_ref.clean(wide, res3, model3, 0.5, 0.0, 1, patch=1)
    want3 = np.zeros((5, 5))
    want3[1:4, 1:4] = -0.5
    want3[2, 2] = 2.0
    assert np.array_equal(res3, want3)
    res3[0, 0] = np.nan
    assert np.array_equal(clean_ref.clean(wide, res3, model3, 0.5, 0.0, 0), [0.0, 2.0, 12.0, 0.0])
    assert np.isnan(clean_ref.clean(wide, np.full((5, 5), np.nan), model3, 0.5, 0.0, 3)[1])


def test_generated_psf_peaks_at_the_centre_for_even_and_odd_sizes():
    for N in (16, 15):
        psf = clean_ref.make_psf(N, 3, fill=0.3)
        assert psf[N // 2, N // 2] == 1.0 and np.abs(psf).max() == 1.0
        img, src = clean_ref.make_sky(psf, 4, nsrc=3)
        assert img.shape == (N, N) and len(src) == 3


# ---- what the Python methods hand to the ABI ------------------------------------------------------------------------------
@pytest.fixture
def rig():
    import gridhip
    rec = Recorder()
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = rec, HANDLE, 0

    def run(fn, name, *spec, handle=HANDLE):
        before = len(rec.calls)
        rec.expect(name, handle, spec)
        out = fn()
        assert rec.calls[before:] == [name], f"{name}: the calls were {rec.calls[before:]}"
        return out
    yield ctx, rec, run
    ctx._h = None


class Zeros:
    """the argument addresses n float64 zeros (a model the method made itself); the recorder writes 1, 2, 3 ... there"""

    def __init__(self, n):
        self.out = Out(f64, n)

    def check(self, arg, where):
        from test_binding_marshalling import memory
        assert np.all(memory(address(arg), f64, self.out.fill.size) == 0.0), f"{where}: not zeros"
        self.out.check(arg, where)


def test_context_clean_host_form(rig):
    ctx, rec, run = rig
    N = 6
    image = np.arange(N * N, dtype=f64).reshape(N, N)
    psf = np.arange(2 * N * N, dtype=np.float32).reshape(N, 2 * N)[:, ::2]  # float32 and non-contiguous: converted
    model = np.ones((N, N))
    st = Out(f64, 4)
    m, r, s = run(lambda: ctx.clean(image, psf, gain=0.25, threshold=0.5, niter=7, border=1, patch=2, model=model),
                  "gridhip_clean", N, Arr(psf, f64), Same(image), Same(model), 0.25, 0.5, 7, 1, 2, st)
    assert m is model and r is image and st.returned(s, (4,))
    # defaults; a model of the method's own: zeros, N x N, returned
    z, st = Zeros(N * N), Out(f64, 4)
    m, r, s = run(lambda: ctx.clean(image, psf), "gridhip_clean", N, Arr(psf, f64), Same(image), z, 0.1, 0.0, 100, 0, 0, st)
    assert r is image and z.out.returned(m, (N, N)) and st.returned(s, (4,))
    # a psf in the right form goes by its own address; integers become the doubles the ABI takes
    right = np.zeros((N, N))
    run(lambda: ctx.clean(image, right, 1, 2, 3.0, 1, 0, model), "gridhip_clean", N, Same(right), Same(image), Same(model),
        1.0, 2.0, 3, 1, 0, Out(f64, 4))


def test_context_clean_refusals_come_before_any_call(rig):
    ctx, rec, run = rig
    N = 6
    image, psf = np.zeros((N, N)), np.zeros((N, N))
    bad = [
        lambda: ctx.clean(image.astype(np.float32), psf),               # the image is updated in place: no conversion
        lambda: ctx.clean(np.zeros((N, 2 * N))[:, ::2], psf),           # not contiguous
        lambda: ctx.clean([[0.0] * N] * N, psf),                        # not an array
        lambda: ctx.clean(np.zeros((N, N + 1)), np.zeros((N, N + 1))),  # not square
        lambda: ctx.clean(np.zeros(N * N), np.zeros(N * N)),
        lambda: ctx.clean(image, np.zeros((N + 1, N + 1))),             # psf of another size
        lambda: ctx.clean(image, psf, model=np.zeros((N, N), dtype=np.float32)),
        lambda: ctx.clean(image, psf, model=np.zeros((N - 1, N - 1))),
        lambda: ctx.clean(image, psf, model=np.zeros((2 * N, N))[::2]),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert rec.calls == [], f"refusal {k} came after {rec.calls}"


@pytest.fixture
def torch_rig(rig, monkeypatch):
    """Tensors of torch on the CPU stand in for cuda tensors: the device back end's `is_cuda` test is lifted and the
    binding to torch's stream recorded instead of made, so that the _dev forms' marshalling runs without a device."""
    import torch
    import gridhip
    from gridhip import _marshal
    ctx, rec, run = rig
    be = _marshal.device()
    monkeypatch.setattr(_marshal._Device, "ok", staticmethod(lambda x, dt: isinstance(x, torch.Tensor) and x.dtype == dt
                                                             and x.is_contiguous()))
    bound = []
    monkeypatch.setattr(gridhip.Context, "_use_torch_stream", lambda self: bound.append(self))
    im = gridhip.Imager(ctx, C.c_void_p(0xBEEF), 5, 6, torch.device("cpu"))
    yield ctx, im, rec, run, bound, be
    im._h = None


class SameT:
    """the argument is the address of the caller's own tensor"""

    def __init__(self, t):
        self.t = t

    def check(self, arg, where):
        assert address(arg) == self.t.data_ptr(), f"{where}: not the caller's tensor"


def tensor_returned(out, t, shape):
    import torch
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == tuple(shape)
    assert t.is_contiguous() and np.array_equal(t.numpy().ravel(), out.fill)
    return True


def test_context_clean_device_form(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N = 6
    image = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    psf32 = torch.arange(N * N, dtype=torch.float32).reshape(N, N)
    model = torch.ones((N, N), dtype=torch.float64)
    st = Out(f64, 4)
    m, r, s = run(lambda: ctx.clean(image, psf32, 0.25, 0.5, 7, 1, 2, model), "gridhip_clean_dev", N,
                  Arr(psf32.numpy(), f64), SameT(image), SameT(model), 0.25, 0.5, 7, 1, 2, st)
    assert m is model and r is image and tensor_returned(st, s, (4,)) and bound == [ctx]
    z, st = Zeros(N * N), Out(f64, 4)
    m, r, s = run(lambda: ctx.clean(image, psf32), "gridhip_clean_dev", N, Arr(psf32.numpy(), f64), SameT(image), z,
                  0.1, 0.0, 100, 0, 0, st)
    assert tensor_returned(z.out, m, (N, N)) and tensor_returned(st, s, (4,))
    for call in (lambda: ctx.clean(image.to(torch.float32), psf32), lambda: ctx.clean(image, psf32, model=np.zeros((N, N))),
                 lambda: ctx.clean(image.t(), psf32)):
        with pytest.raises(ValueError):
            call()
    assert rec.calls.count("gridhip_clean_dev") == 2


def test_imager_clean_and_deconvolve(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, n, h = im.N, im.n, im._h
    image = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    model = torch.ones((N, N), dtype=torch.float64)
    vis = torch.arange(n, dtype=torch.float64).to(torch.complex128)
    st = Out(f64, 4)
    m, r, s = run(lambda: im.clean(image, model, 0.25, 0.5, 7, 1, 2), "gridhip_imager_clean_dev", SameT(image),
                  SameT(model), 0.25, 0.5, 7, 1, 2, st, handle=h)
    assert m is model and r is image and tensor_returned(st, s, (4,)) and bound == [ctx]
    z, st = Zeros(N * N), Out(f64, 4)
    m, r, s = run(lambda: im.clean(image), "gridhip_imager_clean_dev", SameT(image), z, 0.1, 0.0, 100, 0, 0, st, handle=h)
    assert tensor_returned(z.out, m, (N, N)) and r is image

    st, oi = Out(f64, 3 * 4), Out(f64, N * N)
    m, img, s = run(lambda: im.deconvolve(vis, 3, model=model, gain=0.25, threshold=0.5, niter=7, border=1, patch=2),
                    "gridhip_imager_deconvolve_dev", SameT(vis), SameT(model), oi, 3, 0.25, 0.5, 7, 1, 2, st, handle=h)
    assert m is model and tensor_returned(oi, img, (N, N)) and tensor_returned(st, s, (3, 4))
    z, st = Zeros(N * N), Out(f64, 2 * 4)
    m, img, s = run(lambda: im.deconvolve(vis, 2, out=image), "gridhip_imager_deconvolve_dev", SameT(vis), z, SameT(image),
                    2, 0.1, 0.0, 100, 0, 0, st, handle=h)
    assert img is image and tensor_returned(z.out, m, (N, N)) and tensor_returned(st, s, (2, 4))

    before = len(rec.calls)
    bad = [
        lambda: im.clean(image.to(torch.float32)),
        lambda: im.clean(image[:5, :5].contiguous()),
        lambda: im.clean(image.t()),
        lambda: im.clean(image, model=model.to(torch.float32)),
        lambda: im.clean(image, model=torch.zeros((N, N + 1), dtype=torch.float64)),
        lambda: im.deconvolve(vis[:-1], 2),
        lambda: im.deconvolve(vis.to(torch.complex64), 2),
        lambda: im.deconvolve(vis, -1),
        lambda: im.deconvolve(vis, 2, model=model.to(torch.float32)),
        lambda: im.deconvolve(vis, 2, out=torch.zeros((N + 1, N + 1), dtype=torch.float64)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"
