"""Reprojection and mosaicking (gridhip_mosaic[_dev], gridhip_reproject[_dev]), the checks that need no GPU: the library,
the header, the ctypes table, the Haskell imports and the Python surface carry the four entry points; the header states
the rule; a NULL context is refused whatever else is passed and the binding refuses wrong arguments before any call;
facet_grid's geometry; and the numpy restatement the GPU tests compare with (tests/mosaic_ref.py) has the properties the
rule promises and the accuracy of its interpolators against an analytic sky."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mosaic_ref as M
from conftest import ROOT

NAMES = ["gridhip_mosaic", "gridhip_mosaic_dev", "gridhip_reproject", "gridhip_reproject_dev"]
f64 = np.float64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_four():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_mosaic"] == _lib.SIGNATURES["gridhip_mosaic_dev"]
    assert _lib.SIGNATURES["gridhip_reproject"] == _lib.SIGNATURES["gridhip_reproject_dev"]
    # R is an array of the form's own kind: device memory in the _dev form
    assert _lib.SIGNATURES["gridhip_mosaic_dev"][1][6] is C.c_void_p and _lib.SIGNATURES["gridhip_reproject_dev"][1][4] is C.c_void_p
    assert len(_lib.SIGNATURES["gridhip_mosaic"][1]) == 18 and len(_lib.SIGNATURES["gridhip_reproject"][1]) == 12
    assert _lib.load().gridhip_version() >= 290
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 290
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in hs, name


def test_header_states_the_rule():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("reprojection and mosaicking"):raw.index("int gridhip_mosaic(")]
    for phrase in ("l = theta (x - N/2) / N", "from the DESTINATION frame to facet f's frame", "DEVICE memory in the _dev",
                   "R22 <= 0", "|R R^T - I| above 1e-9", "contraction is off", "BEYOND THE HORIZON", "n = sqrt(1 - r2)",
                   "l' = (R00 l + R01 m) + R02 n", "If not n' > 0", "fx = (l' * Ns) / theta_s + (double)(Ns/2)",
                   "t = (outer - d) / (outer - inner)", "s(d) = (t t) (3 - 2 t)", "floor(0.5 + fx)", "a (1 - t) + b t",
                   "c0 = ((-0.5 t + 1) t - 0.5) t", "c1 = ((1.5 t - 2.5) t) t + 1", "c2 = ((-1.5 t + 2) t + 0.5) t",
                   "c3 = ((0.5 t - 0.5) t) t", "((c0 a + c1 b) + c2 c) + c3 d", "ALL TAPS", "LEFT OUT", "not finite or not > 0",
                   "num = num + w v, den = den + w", "CONTRIBUTES NOTHING", "den > wmin", "wsum = +0.0", "F above 4096",
                   "32768", "GRIDHIP_EUNSUPPORTED", "no memset node", "captured into a graph", "16 x 16 tiles", "in ascending order",
                   '"mosaic_cull"', "DETERMINISM", "no floating-point atomic", "integer atomics", "OUT OF SCOPE"):
        assert phrase in section, phrase


def test_python_surface():
    import gridhip
    for owner, name in ((gridhip.Context, "mosaic"), (gridhip.Context, "reproject"), (gridhip, "facet_grid")):
        assert callable(getattr(owner, name)), name
    assert "facet_grid" in gridhip.__all__


def test_null_context_is_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_mosaic.py::test_refusals); here: a NULL context is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    F, Ns, Nd = 2, 4, 5
    fac, R = np.full((F, Ns, Ns), 2.0), np.tile(np.eye(3).ravel(), (F, 1))
    out, ws, st = np.full((Nd, Nd), 5.0), np.full((Nd, Nd), 6.0), np.full(8, 7.0)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for fn in (lib.gridhip_mosaic, lib.gridhip_mosaic_dev):
        for FF, kind, th in ((F, 3, 0.1), (0, 3, 0.1), (F, 2, 0.1), (F, 3, -1.0), (1 << 20, 1, 0.1)):
            assert fn(None, FF, Ns, th, p(fac), None, p(R), kind, 2.0, 2.0, 1, 0.0, 0.0, Nd, 0.2, p(out), p(ws), p(st)) == _lib.EINVAL
    for fn in (lib.gridhip_reproject, lib.gridhip_reproject_dev):
        for kind in (3, 7):
            assert fn(None, Ns, 0.1, p(fac), p(R), kind, 2.0, 2.0, 0.0, Nd, 0.2, p(out)) == _lib.EINVAL
    for a, val in ((fac, 2.0), (out, 5.0), (ws, 6.0), (st, 7.0)):
        assert np.all(a == val)
    assert np.array_equal(R, np.tile(np.eye(3).ravel(), (F, 1)))


class _NoCalls:
    """stands in for the loaded library: any entry point that is reached is an error"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_the_binding_refuses_before_any_call():
    import gridhip
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = _NoCalls(), C.c_void_p(1), 0
    try:
        fac, R = np.zeros((2, 8, 8)), np.tile(np.eye(3).ravel(), (2, 1))
        good = dict(facets=fac, theta_src=0.1, R=R, theta_dst=0.2, N_dst=16)
        Rbad, Rnan, Rskew = R.copy(), R.copy(), R.copy()
        Rbad[1] = np.diag([1.0, -1.0, -1.0]).ravel()  # a rotation, but R22 <= 0
        Rnan[0, 4] = np.nan
        Rskew[1, 0] = 1.0 + 1e-6
        for change in (dict(facets=np.zeros((2, 8, 7))), dict(facets=np.zeros(8)), dict(facets=np.zeros((2, 8, 8), dtype=complex)),
                       dict(R=R[:1]), dict(R=Rbad), dict(R=Rnan), dict(R=Rskew), dict(kind="lanczos"), dict(kind=3),
                       dict(theta_src=0.0), dict(theta_dst=np.inf), dict(N_dst=0), dict(window=(3.0, 2.0)),
                       dict(window=(-1.0, 2.0)), dict(window=(1.0, np.inf)), dict(wmin=-1.0), dict(wmin=np.nan),
                       dict(weights=np.zeros((2, 8, 9))), dict(out=np.zeros((16, 15))), dict(out=np.zeros((16, 16), dtype=np.float32))):
            with pytest.raises(ValueError):
                ctx.mosaic(**{**good, **change})
        with pytest.raises(ValueError):
            ctx.reproject(fac, 0.1, np.eye(3), 0.2, 16)  # (one image, not a stack)
        with pytest.raises(ValueError):
            ctx.reproject(fac[0], 0.1, Rbad[1], 0.2, 16)
        with pytest.raises(AssertionError, match="gridhip_mosaic was called"):
            ctx.mosaic(**good)  # (and good arguments do reach the library)
        with pytest.raises(AssertionError, match="gridhip_reproject was called"):
            ctx.reproject(fac[0], 0.1, np.eye(3), 0.2, 16)
    finally:
        ctx._h = None


# ---- facet_grid -----------------------------------------------------------------------------------------------------------
def test_facet_grid_geometry():
    import gridhip
    theta, nf, ov, N = 0.2, 3, 0.25, 64
    centres, R, theta_f, (inner, outer) = gridhip.facet_grid(theta, nf, ov, N)
    assert centres.shape == (9, 2) and R.shape == (9, 9) and R.dtype == f64
    c = theta * ((np.arange(nf) + 0.5) / nf - 0.5)
    for j in range(nf):
        for i in range(nf):
            f = j * nf + i
            assert centres[f, 0] == c[i] and centres[f, 1] == c[j]
            l0, m0 = centres[f]
            assert np.array_equal(R[f, 6:], [l0, m0, np.sqrt(1.0 - (l0 * l0 + m0 * m0))])  # the third row: the centre itself
            assert M.rotation_ok(R[f]) and np.array_equal(R[f], gridhip.rotation_to(l0, m0).ravel())
    assert centres[4, 0] == 0.0 and centres[4, 1] == 0.0 and np.array_equal(R[4], np.eye(3).ravel())
    assert theta_f == (theta / nf) * (1 + ov)
    D = N / (1 + ov)  # cells between neighbouring centres
    assert abs((inner + outer) - D) <= 2 * np.spacing(D) and 0 < inner < outer
    assert N / 2 - outer >= 2.0  # room for the cubic's taps at every edge
    # along a seam a point d cells from one centre lies D - d from the next: the two feathers sum to 1
    d = np.linspace(inner, outer, 1001)
    tot = M.feather(d, inner, outer) + M.feather(D - d, inner, outer)
    assert np.abs(tot - 1.0).max() <= 8 * np.finfo(f64).eps
    # inside `inner` one facet alone, at full weight
    assert np.all(M.feather(np.linspace(0, inner, 50), inner, outer) == 1.0) and M.feather(f64(D), inner, outer) == 0.0
    # N = 1: the window as fractions of the facet's side
    _, _, _, (i1, o1) = gridhip.facet_grid(theta, nf, ov)
    assert abs(i1 * N - inner) <= 4 * np.spacing(inner) and abs(o1 * N - outer) <= 4 * np.spacing(outer)
    # no overlap: a hard window at the facet's edge
    _, _, tf0, (i0, o0) = gridhip.facet_grid(theta, 2, 0.0, N)
    assert tf0 == theta / 2 and i0 == o0 == N / 2
    for bad in (dict(theta=0.0), dict(nf=0), dict(overlap=-0.1), dict(N=0)):
        with pytest.raises(ValueError):
            gridhip.facet_grid(**{**dict(theta=0.1, nf=2), **bad})


# ---- properties of the restatement ------------------------------------------------------------------------------------------
RNG = np.random.default_rng(290)


@pytest.mark.parametrize("kind,low,high", [("nearest", 0, 0), ("bilinear", 0, 1), ("cubic", 1, 2)])
def test_identity_returns_the_sources_bits(kind, low, high):
    """R = I, equal theta and N: with a dyadic theta every step of the map is exact, fx = x and t = 0, and the interpolators
    return the tap itself - c1 = 1 and the other coefficients are zeros.  Inside the tap border only: the bilinear reaches
    one cell past x, the cubic one before it and two past it."""
    N, theta = 32, 0.125
    src = RNG.normal(size=(N, N))  # (no zero among them: -0 + 0 would lose its sign)
    out = M.reproject(src, theta, np.eye(3), theta, N, kind, window=(N, N))
    lo, hi = low, N - high
    assert M.same_bits(out[lo:hi, lo:hi], src[lo:hi, lo:hi])
    blank = np.ones((N, N), dtype=bool)
    blank[lo:hi, lo:hi] = False
    assert np.isnan(out[blank]).all()


@pytest.mark.parametrize("kind", ["nearest", "bilinear", "cubic"])
def test_constant_facets_give_the_constant(kind):
    """The interpolation weights of a row sum to 1 within an ulp or two and num / den cancels the feather: 4 ulps."""
    import gridhip
    centres, R, theta_f, win = gridhip.facet_grid(0.2, 2, 0.3, 24)
    c = 1.2345678901234567
    out, wsum, st = M.mosaic(np.full((4, 24, 24), c), theta_f, R, 0.2, 40, kind, window=win)
    cov = wsum > 0
    assert cov.sum() > 0.8 * 40 * 40 and st[5] == 4 and st[0] == cov.sum()
    assert np.abs(out[cov] - c).max() <= 4 * np.spacing(c)
    assert np.isnan(out[~cov]).all()


def test_nan_under_a_zero_weight_does_not_appear():
    import gridhip
    N = 16
    fac = RNG.normal(size=(2, N, N))
    wt = np.ones((2, N, N))
    fac[0, 4:9, 4:9] = np.nan   # under zero, negative and NaN weights
    wt[0, 3:10, 3:6] = 0.0
    wt[0, 3:10, 6:8] = -1.0
    wt[0, 3:10, 8:10] = np.nan
    R = np.array([np.eye(3).ravel(), gridhip.rotation_to(0.001, -0.002).ravel()])
    out, wsum, st = M.mosaic(fac, 0.1, R, 0.1, N, "bilinear", weights=wt, blank=-7.0)
    assert np.isfinite(out).all()
    assert st[4] > 0  # (step 5 comes before step 6: a tap that is not finite is counted whatever the weight under it)
    assert (out == -7.0).sum() == st[1] and st[0] + st[1] == N * N
    # without the weights the same NaNs are left out and counted, and still do not reach the output
    out2, _, st2 = M.mosaic(fac, 0.1, R, 0.1, N, "bilinear", blank=-7.0)
    assert np.isfinite(out2).all() and st2[4] == st[4]
    # outside the window too
    far = fac[1:].copy()
    far[0, :5, :] = np.inf  # (the window keeps the cells 7 .. 9 about the centre cell 8)
    out3, _, st3 = M.mosaic(far, 0.1, R[:1], 0.1, N, "nearest", window=(1.0, 1.0), blank=-7.0)
    assert st3[4] == 0 and st3[0] == 9 and np.isfinite(out3).all()


def test_horizon_cells_are_blank():
    N = 33
    out, wsum, st = M.mosaic(np.ones((1, N, N)), 2.2, np.eye(3), 2.2, N, "nearest", blank=-1.0)
    lc = M.cell_coords(N, 2.2)
    l, m = np.meshgrid(lc, lc)
    beyond = ~(l * l + m * m < 1.0)
    assert beyond[0, 0] and beyond[-1, -1] and not beyond[N // 2, N // 2]
    assert np.all(out[beyond] == -1.0) and np.all(wsum[beyond] == 0.0) and np.all(out[~beyond] == 1.0)


def test_a_refused_facet_contributes_nothing():
    fac = np.stack([np.full((8, 8), 1.0), np.full((8, 8), 100.0), np.full((8, 8), 3.0)])
    R = np.tile(np.eye(3).ravel(), (3, 1))
    R[1, 8] = -1.0
    out, wsum, st = M.mosaic(fac, 0.1, R, 0.1, 8, "nearest", normalize=False)
    assert st[2] == 2 and st[3] == 1 and st[5] == 2 and np.nanmax(out) == 4.0 and np.nanmax(wsum) == 2.0


# ---- accuracy against an analytic sky ---------------------------------------------------------------------------------------
def _sky(l, m, n, srcs, sig):
    """Gaussians on the sphere: exp(-chord^2 / 2 sig^2) about each direction (a, b, sqrt(1 - a^2 - b^2))"""
    out = 0.0
    for a, b, s in srcs:
        c = np.sqrt(1 - a * a - b * b)
        out = out + s * np.exp(-((l - a) ** 2 + (m - b) ** 2 + (n - c) ** 2) / (2 * sig * sig))
    return out


def _dirs(N, theta):
    lc = M.cell_coords(N, theta)
    l, m = np.meshgrid(lc, lc)
    return l, m, np.sqrt(1 - l * l - m * m)


def test_accuracy_against_an_analytic_sky(capsys):
    """One facet of 64^2 cells, theta_s = 0.05, about (0.02, -0.015), reprojected onto 128^2 cells of theta_d = 0.1; three
    Gaussians of FWHM 6 facet cells, the sky evaluated in closed form at the facet's cells and at the destination's.  The
    bounds are the restatement's own errors on this case, times 1.5."""
    import gridhip
    Ns, ths, Nd, thd, l0, m0 = 64, 0.05, 128, 0.1, 0.02, -0.015
    R = gridhip.rotation_to(l0, m0)
    srcs = [(0.02, -0.015, 1.0), (0.03, -0.005, 0.7), (0.008, -0.027, -0.4)]
    sig = 6 * (ths / Ns) / 2.3548
    lf, mf, nf = _dirs(Ns, ths)  # the facet's cells in its own frame; R^T takes them to the destination frame
    facet = _sky(R[0, 0] * lf + R[1, 0] * mf + R[2, 0] * nf, R[0, 1] * lf + R[1, 1] * mf + R[2, 1] * nf,
                 R[0, 2] * lf + R[1, 2] * mf + R[2, 2] * nf, srcs, sig)
    truth = _sky(*_dirs(Nd, thd), srcs, sig)
    err = {}
    for kind in ("nearest", "bilinear", "cubic"):
        out = M.reproject(facet, ths, R, thd, Nd, kind)
        ok = ~np.isnan(out)
        assert ok.sum() > 900  # (the facet covers a quarter of the destination's side: 32^2 cells less the tap border)
        err[kind] = np.abs(out - truth)[ok].max()
    with capsys.disabled():
        print("mosaic accuracy, maximum error in units of the peak:", {k: float(f"{v:.3e}") for k, v in err.items()})
    assert err["cubic"] <= 1.5 * 2.835e-3      # measured 2.835e-3
    assert err["bilinear"] <= 1.5 * 2.875e-2   # measured 2.875e-2 (nearest: 1.061e-1)
    assert err["cubic"] < err["bilinear"] < err["nearest"]
