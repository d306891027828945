"""The restoring beam and the restore (gridhip_fit_beam*, gridhip_restore*, gridhip_imager_beam_dev,
gridhip_imager_restore_dev), the checks that need no GPU: the library, the header, the ctypes table, both bindings and
the hpp carry the six entry points; a NULL context or imager is refused with GRIDHIP_EINVAL whatever else is passed;
Context.fit_beam, Context.restore, Imager.beam and Imager.restore hand the ABI the right pointers, shapes, scalar order
and beam buffer (against the recording library of test_binding_marshalling.py) and refuse wrong dtypes and shapes
before any call; and the numpy restatement the GPU tests compare with (tests/restore_ref.py) is right on cases computed
by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clean_ref
import restore_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same, address

NAMES = ["gridhip_fit_beam", "gridhip_fit_beam_dev", "gridhip_restore", "gridhip_restore_dev", "gridhip_imager_beam_dev",
         "gridhip_imager_restore_dev"]
f64 = np.float64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_restore():
    from gridhip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gridhip.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_fit_beam"] == _lib.SIGNATURES["gridhip_fit_beam_dev"]
    assert _lib.SIGNATURES["gridhip_restore"] == _lib.SIGNATURES["gridhip_restore_dev"]
    assert _lib.load().gridhip_version() >= 170


def test_bindings_carry_the_restore():
    import gridhip
    for owner, method in ((gridhip.Context, "fit_beam"), (gridhip.Context, "restore"), (gridhip.Imager, "beam"),
                          (gridhip.Imager, "restore")):
        assert callable(getattr(owner, method)), method
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("fitBeamIO", "restoreIO", "imagerBeamIO", "imagerRestoreIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bfit_beam\s*\(", hpp) and "gridhip_fit_beam" in hpp
    assert re.search(r"\brestore\s*\(", hpp) and "gridhip_restore" in hpp


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_restore.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    N = 4
    arrs = [np.full(N * N, v) for v in (1.0, 2.0, 3.0)]
    beam = np.full(8, 7.0)
    m, r, o = (C.c_void_p(a.ctypes.data) for a in arrs)
    b = C.c_void_p(beam.ctypes.data)
    for window, cut in [(8, 0.5), (0, 0.5), (-1, 0.5), (8, 0.0), (8, 1.0), (8, float("nan"))]:
        assert lib.gridhip_fit_beam(None, N, m, window, cut, b) == _lib.EINVAL
        assert lib.gridhip_fit_beam_dev(None, N, m, window, cut, b) == _lib.EINVAL
        assert lib.gridhip_imager_beam_dev(None, window, cut, b) == _lib.EINVAL
        for support in (4, 0, 33):
            assert lib.gridhip_imager_restore_dev(None, m, r, window, cut, support, o, b) == _lib.EINVAL
            assert lib.gridhip_imager_restore_dev(None, m, r, window, cut, support, o, None) == _lib.EINVAL
    for support in (4, 0, -1, 33):
        assert lib.gridhip_restore(None, N, m, r, b, support, o) == _lib.EINVAL
        assert lib.gridhip_restore_dev(None, N, m, r, b, support, o) == _lib.EINVAL
    for n_, mm, rr, bb, oo in ((0, m, r, b, o), (N, None, r, b, o), (N, m, None, b, o), (N, m, r, None, o),
                               (N, m, r, b, None), (N, m, r, b, m)):
        assert lib.gridhip_restore(None, n_, mm, rr, bb, 4, oo) == _lib.EINVAL
    assert lib.gridhip_fit_beam(None, N, None, 8, 0.5, b) == _lib.EINVAL
    assert lib.gridhip_fit_beam(None, N, m, 8, 0.5, None) == _lib.EINVAL
    for a, v in zip(arrs, (1.0, 2.0, 3.0)):
        assert np.all(a == v)
    assert np.all(beam == 7.0)


# ---- the numpy restatement on cases computed by hand ---------------------------------------------------------------------
def gaussian(N, A, B, Cq):
    c = N // 2
    yy, xx = np.mgrid[0:N, 0:N]
    dy, dx = (yy - c).astype(f64), (xx - c).astype(f64)
    return np.exp(-(A * dx * dx + 2.0 * B * dx * dy + Cq * dy * dy))


@pytest.mark.parametrize("N", [33, 32])
def test_an_exact_sampled_gaussian_returns_its_own_form(N):
    """ln p is exactly quadratic in (dx, dy), so the weighted fit has zero residual whatever cells take part"""
    for A, B, Cq in ((0.11, 0.0, 0.11), (0.05, 0.01, 0.02), (0.3, -0.1, 0.2), (2.0, 0.5, 1.5)):
        for window, cut in ((8, 0.5), (3, 0.1), (12, 0.9)):
            b = restore_ref.fit_beam(gaussian(N, A, B, Cq), window, cut)
            assert b[7] == 1.0 and b[6] >= 3, (A, B, Cq, window, cut, b)
            scale = max(A, Cq)
            assert max(abs(b[0] - A), abs(b[1] - B), abs(b[2] - Cq)) <= 1e-12 * scale, (A, B, Cq, window, cut, b)


def test_a_rotated_ellipse_returns_its_axes_and_angle():
    """FWHMs 9 and 4 cells, the major axis at 30 degrees from +x towards +y: A, B, C follow from rotating
    diag(lmaj, lmin), lambda = 4 ln 2 / FWHM^2"""
    for deg in (30.0, -60.0, 90.0, 0.0, 89.0):
        phi = math.radians(deg)
        lmaj, lmin = 4 * math.log(2) / 81.0, 4 * math.log(2) / 16.0
        cs, sn = math.cos(phi), math.sin(phi)
        A = lmaj * cs * cs + lmin * sn * sn
        Cq = lmaj * sn * sn + lmin * cs * cs
        B = (lmaj - lmin) * cs * sn
        b = restore_ref.fit_beam(gaussian(41, A, B, Cq), 10, 0.3)
        assert b[7] == 1.0
        assert abs(b[3] - 9.0) < 1e-9 and abs(b[4] - 4.0) < 1e-9, b
        assert abs(b[5] - phi) < 1e-9 and -math.pi / 2 < b[5] <= math.pi / 2, (deg, b[5])
    b = restore_ref.fit_beam(gaussian(21, 0.2, 0.0, 0.2), 5, 0.2)  # circular: the angle is 0 by definition
    assert b[5] == 0.0 and abs(b[3] - b[4]) < 1e-12 and b[3] >= b[4]


def test_which_cells_take_part():
    """a 7 x 7 PSF by hand: the eight neighbours take part when positive even below the cut; farther cells only at or
    above it; a cell above 1 or NaN never"""
    psf = np.zeros((7, 7))
    psf[3, 3] = 2.0
    psf[2:5, 2:5] = 0.2   # neighbours: p = 0.1, below the cut, positive
    psf[3, 3] = 2.0
    psf[3, 5] = 1.2       # p = 0.6 at distance 2: at or above the cut
    psf[1, 3] = 0.2       # p = 0.1 at distance 2: below it
    psf[3, 1] = 3.0       # p = 1.5: above 1
    psf[5, 3] = np.nan
    M, g, ncells, pc = restore_ref.normal_equations(psf, 3, 0.5)
    assert ncells == 9 and pc == 2.0
    psf[2, 2] = -0.2      # a non-positive neighbour has no logarithm
    psf[2, 3] = np.nan
    assert restore_ref.normal_equations(psf, 3, 0.5)[2] == 7
    assert restore_ref.normal_equations(psf, 1, 0.5)[2] == 6  # the window cuts the far cell off


def test_a_psf_without_usable_neighbours_fails():
    psf = np.full((9, 9), -0.1)
    psf[4, 4] = 1.0
    b = restore_ref.fit_beam(psf, 4, 0.5)
    assert b[7] == 0.0 and b[6] == 0.0 and np.all(np.isnan(b[:6]))
    psf[4, 5] = psf[4, 3] = 0.5  # two cells: fewer than three
    b = restore_ref.fit_beam(psf, 4, 0.5)
    assert b[7] == 0.0 and b[6] == 2.0 and np.all(np.isnan(b[:6]))
    for centre in (0.0, -1.0, np.nan, np.inf):
        psf = gaussian(9, 0.3, 0.0, 0.3)
        psf[4, 4] = centre
        b = restore_ref.fit_beam(psf, 4, 0.5)
        assert b[7] == 0.0 and np.all(np.isnan(b[:6])), centre
    # a saddle: the cells with p <= 1 fit A = 0.3, C = -0.05 exactly, which is not positive definite
    saddle = gaussian(9, 0.3, 0.0, -0.05)
    b = restore_ref.fit_beam(saddle, 4, 0.5)
    assert b[7] == 0.0 and b[6] >= 3 and np.all(np.isnan(b[:6]))
    assert not restore_ref.beam_usable([1.0, 2.0, 1.0, 0, 0, 0, 8, 1.0])  # A C - B^2 < 0
    assert not restore_ref.beam_usable([1.0, 0.0, 1.0, 0, 0, 0, 8, 0.0])  # ok = 0
    assert restore_ref.beam_usable([1.0, 0.5, 1.0, 0, 0, 0, 8, 1.0])


def test_a_single_component_restores_to_the_sampled_beam():
    N, s = 17, 3
    beam = np.array([0.3, 0.1, 0.2, 0, 0, 0, 8, 1.0])
    model = np.zeros((N, N))
    model[8, 6] = 2.0
    model[0, 16] = -1.0  # a corner: the beam is clipped by two edges
    res = np.full((N, N), 0.25)
    out, mag = restore_ref.restore(model, res, beam, s)
    want, wmag = res.copy(), np.abs(res)
    for (y0, x0), f in (((8, 6), 2.0), ((0, 16), -1.0)):
        for dy in range(-s, s + 1):
            for dx in range(-s, s + 1):
                y, x = y0 + dy, x0 + dx
                if 0 <= y < N and 0 <= x < N:
                    w = math.exp(-(0.3 * dx * dx + 2 * 0.1 * dx * dy + 0.2 * dy * dy))
                    want[y, x] += f * w
                    wmag[y, x] += abs(f) * w
    assert np.abs(out - want).max() < 1e-15 and np.abs(mag - wmag).max() < 1e-15
    assert out[8, 6] == 2.25 and out[0, 16] == -0.75
    assert out[8, 6 + s + 1] == 0.25 and out[8 + 1, 6 + 1] == 0.25 + 2.0 * math.exp(-(0.3 + 0.2 + 0.2))
    # an empty model: residual + 0.0, so that a -0.0 residual comes back as +0.0
    res[3, 3] = -0.0
    out, _ = restore_ref.restore(np.zeros((N, N)), res, beam, s)
    assert np.array_equal(out, res) and not np.signbit(out[3, 3])
    assert np.all(np.isnan(restore_ref.restore(model, res, [np.nan] * 6 + [0.0, 0.0], s)[0]))


def test_generated_psfs_are_fitted_as_the_issue_states():
    for N in (255, 256):
        b = restore_ref.fit_beam(restore_ref.smooth_psf(N, 1, 0.15), 8, 0.5)
        assert b[7] == 1.0 and b[6] == 20 and abs(b[3] - 5.0) < 0.1 and abs(b[4] - 5.0) < 0.1, b
        b = restore_ref.fit_beam(restore_ref.smooth_psf(N, 1, 0.1, 0.5, 0.3), 8, 0.5)
        assert b[7] == 1.0 and b[6] == 88 and abs(b[3] - 15.0) < 0.2 and abs(b[4] - 7.5) < 0.1, b
    for N in (256, 255, 600):
        for seed in (1, 2, 3):
            b = restore_ref.fit_beam(clean_ref.make_psf(N, seed), 8, 0.5)
            assert b[7] == 1.0 and b[6] == 8 and 1.4 < b[4] <= b[3] < 1.8, (N, seed, b)


def test_support_from_a_beam():
    from gridhip._marshal import beam_support
    lam = 0.1
    R = beam_support([lam, 0.0, 0.3, 0, 0, 0, 8, 1.0])
    assert math.exp(-lam * R * R) <= 1e-9 < math.exp(-lam * (R - 1) ** 2) and R == 15
    assert beam_support([5.0, 0.0, 5.0, 0, 0, 0, 8, 1.0]) == 3
    with pytest.raises(ValueError):
        beam_support([0.01, 0.0, 0.3, 0, 0, 0, 8, 1.0])  # 46 cells
    with pytest.raises(ValueError):
        beam_support([np.nan] * 6 + [2.0, 0.0])


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


BEAM = np.array([0.1, 0.0, 0.3, 5.26, 3.04, 0.0, 20.0, 1.0])  # support 15


def test_context_fit_beam_and_restore_host_form(rig):
    ctx, rec, run = rig
    N = 6
    psf = np.arange(2 * N * N, dtype=np.float32).reshape(N, 2 * N)[:, ::2]  # float32 and non-contiguous: converted
    ob = Out(f64, 8)
    b = run(lambda: ctx.fit_beam(psf, window=5, cut=0.25), "gridhip_fit_beam", N, Arr(psf, f64), 5, 0.25, ob)
    assert ob.returned(b, (8,))
    right = np.zeros((N, N))
    ob = Out(f64, 8)
    run(lambda: ctx.fit_beam(right), "gridhip_fit_beam", N, Same(right), 8, 0.5, ob)

    model = np.arange(N * N, dtype=f64).reshape(N, N)
    res32 = np.ones((N, N), dtype=np.float32)
    oo = Out(f64, N * N)
    out = run(lambda: ctx.restore(model, res32, BEAM, support=4), "gridhip_restore", N, Same(model), Arr(res32, f64),
              Same(BEAM), 4, oo)
    assert oo.returned(out, (N, N))
    # support derived from the beam (15 for lambda_min = 0.1); out = the residual itself, in place; a list for a beam
    res = np.ones((N, N))
    out = run(lambda: ctx.restore(model, res, BEAM.tolist(), out=res), "gridhip_restore", N, Same(model), Same(res),
              Arr(BEAM, f64), 15, Same(res))
    assert out is res


def test_context_refusals_come_before_any_call(rig):
    ctx, rec, run = rig
    N = 6
    model, res = np.zeros((N, N)), np.zeros((N, N))
    bad = [
        lambda: ctx.fit_beam(np.zeros((N, N + 1))),
        lambda: ctx.fit_beam(np.zeros(N * N)),
        lambda: ctx.restore(np.zeros((N, N + 1)), np.zeros((N, N + 1)), BEAM, 4),
        lambda: ctx.restore(model, np.zeros((N + 1, N + 1)), BEAM, 4),
        lambda: ctx.restore(model, res, BEAM[:7], 4),
        lambda: ctx.restore(model, res, BEAM, 4, out=np.zeros((N, N), dtype=np.float32)),  # written in place: no conversion
        lambda: ctx.restore(model, res, BEAM, 4, out=np.zeros((N - 1, N - 1))),
        lambda: ctx.restore(model, res, BEAM, 4, out=np.zeros((2 * N, N))[::2]),
        lambda: ctx.restore(model, res, [np.nan] * 6 + [0.0, 0.0]),        # a failed fit has no support to derive
        lambda: ctx.restore(model, res, [0.01, 0, 0.01, 0, 0, 0, 8, 1]),   # 46 cells: above 32
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert rec.calls == [], f"refusal {k} came after {rec.calls}"


@pytest.fixture
def torch_rig(rig, monkeypatch):
    """Tensors of torch on the CPU stand in for cuda tensors, as in test_clean_host.py"""
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


def test_context_device_forms(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N = 6
    psf = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    ob = Out(f64, 8)
    b = run(lambda: ctx.fit_beam(psf, 4, 0.3), "gridhip_fit_beam_dev", N, SameT(psf), 4, 0.3, ob)
    assert tensor_returned(ob, b, (8,)) and bound == [ctx]
    model, res = torch.ones((N, N), dtype=torch.float64), torch.zeros((N, N), dtype=torch.float64)
    beam = torch.from_numpy(BEAM.copy())
    oo = Out(f64, N * N)
    out = run(lambda: ctx.restore(model, res, beam, 7), "gridhip_restore_dev", N, SameT(model), SameT(res), SameT(beam), 7, oo)
    assert tensor_returned(oo, out, (N, N))
    out = run(lambda: ctx.restore(model, res, beam, out=res), "gridhip_restore_dev", N, SameT(model), SameT(res),
              SameT(beam), 15, SameT(res))
    assert out is res
    with pytest.raises(ValueError):
        ctx.restore(model, res, beam, 7, out=np.zeros((N, N)))
    assert rec.calls.count("gridhip_restore_dev") == 2


def test_imager_beam_and_restore(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, h = im.N, im._h
    ob = Out(f64, 8)
    b = run(lambda: im.beam(5, 0.25), "gridhip_imager_beam_dev", 5, 0.25, ob, handle=h)
    assert tensor_returned(ob, b, (8,)) and bound == [ctx]
    ob = Out(f64, 8)
    run(lambda: im.beam(), "gridhip_imager_beam_dev", 8, 0.5, ob, handle=h)
    model, res = torch.ones((N, N), dtype=torch.float64), torch.zeros((N, N), dtype=torch.float64)
    oo, ob = Out(f64, N * N), Out(f64, 8)
    out, b = run(lambda: im.restore(model, res, support=9, window=5, cut=0.25), "gridhip_imager_restore_dev", SameT(model),
                 SameT(res), 5, 0.25, 9, oo, ob, handle=h)
    assert tensor_returned(oo, out, (N, N)) and tensor_returned(ob, b, (8,))
    ob = Out(f64, 8)
    out, b = run(lambda: im.restore(model, res, 2, out=res), "gridhip_imager_restore_dev", SameT(model), SameT(res), 8, 0.5,
                 2, SameT(res), ob, handle=h)
    assert out is res and tensor_returned(ob, b, (8,))
    before = len(rec.calls)
    bad = [
        lambda: im.restore(model.to(torch.float32), res, 4),
        lambda: im.restore(model, res[:5, :5].contiguous(), 4),
        lambda: im.restore(model.t(), res, 4),
        lambda: im.restore(model, res, 4, out=torch.zeros((N, N + 1), dtype=torch.float64)),
        lambda: im.restore(model, res, 4, out=res.to(torch.float32)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"
