"""Continuum subtraction (gridhip_contsub[_dev], gridhip_contsub_tile), the checks that need no GPU: the library, the
header, the ctypes table and both bindings carry the three entry points; the header states the semantics; a NULL context is
refused whatever else is passed; Context.contsub hands the ABI the right pointers, layout, ncomp and sizes and refuses wrong
arguments before any call; and the numpy restatement the GPU tests compare with (tests/contsub_ref.py) against an
independent solve, on the fall-back rows, and on the clip case - a condition on the definition, checked on the restatement
alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contsub_ref as R
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_contsub", "gridhip_contsub_dev", "gridhip_contsub_tile"]
f64, c128, u8 = np.float64, np.complex128, np.uint8
NAN, INF = np.nan, np.inf
CLIP_SEED = 10  # (the GPU test runs the same case: tests/test_gpu_contsub.py)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_three():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_contsub"] == _lib.SIGNATURES["gridhip_contsub_dev"]
    for macro, value in (("MAX_CHANNELS", 4096), ("MAX_DEGREE", 3), ("ROWINFO", 4), ("STATS", 8)):
        assert int(re.search(rf"#define GRIDHIP_CONTSUB_{macro} (\d+)", src).group(1)) == value, macro


def test_header_states_the_semantics():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("continuum subtraction"):raw.index("int gridhip_contsub(")]
    for phrase in ("[R][C]", "[C][R]", "T_0 = 1, T_1 = x, T_{p+1} = (2 * x) * T_p - T_{p-1}", "p up to 2 * degree",
                   "chan_mask[c] != 0 &&", "isfinite(x[c])",
                   "FLAGGED ON INPUT", "NOT FINITE", "MASKED", "16 + i", "USED",                          # the classes
                   "mu_p = mu_p + w * T_p[c]", "g = w * T_k[c]", "A_jk = 0.5 * (mu_{j+k} + mu_{|j-k|})",   # the product identity
                   "LDL^T without pivoting", "A_kk > 0 and t > 1e-12 * A_kk", "k - 1", "Degree -1",       # the pivot rule
                   "z_k = z_k - L_kp * z_p", "a_k = a_k - L_ik * a_i", "acc = acc + a_k * T_k[c]",
                   "q_c = w * (r.re * r.re + r.im * r.im)", "qbar = Q / (double)n_used", "(nsigma * nsigma) * qbar",
                   "out == data", "[D+1][R][ncomp]", "[4][R]", "GRIDHIP_EUNSUPPORTED", "4096", "2^31 - 1", "three launches",
                   "DETERMINISM", "the two layouts", "NOT HERE", "median", "splines", "fits along time"):
        assert phrase in section, phrase


def test_bindings_carry_the_three():
    import gridhip
    assert callable(gridhip.Context.contsub) and callable(gridhip.contsub_tile) and callable(gridhip.channel_coordinate)
    assert "contsub_tile" in gridhip.__all__ and "channel_coordinate" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_the_tile():
    import gridhip
    rows, chunk = gridhip.contsub_tile()
    assert rows >= 1 and chunk >= 1 and rows % 64 == 0  # (a lane per row: whole waves)
    from gridhip import _lib
    assert _lib.load().gridhip_contsub_tile(None) == _lib.EINVAL


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists: the argument rules themselves are checked on the GPU
    (test_gpu_contsub.py::test_refusals); here a NULL context is GRIDHIP_EINVAL for good and bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    Rr, Cc, D = 3, 5, 2
    n = Rr * Cc
    x, mk, data, wt = np.full(Cc, 0.5), np.full(Cc, 1, dtype=u8), np.full(n, 1 + 2j), np.full(n, 4.0)
    out, co, ri, cd, st = np.full(n, 3 - 1j), np.full(Rr * (D + 1), 7 + 0j), np.full(Rr * 4, 5.0), np.full(n, 9, dtype=u8), np.full(8, 6.0)
    px, pm, pd, pw, po, pc, pr, pcd, ps = (C.c_void_p(a.ctypes.data) for a in (x, mk, data, wt, out, co, ri, cd, st))
    # R, C, layout, ncomp, degree, mode, nsigma, niter
    cases = [(Rr, Cc, 0, 2, D, 0, 0.0, 0), (Rr, Cc, 1, 2, D, 1, 3.0, 4), (0, Cc, 0, 2, D, 0, 0.0, 0), (Rr, 0, 0, 2, D, 0, 0.0, 0),
             (Rr, Cc, 2, 2, D, 0, 0.0, 0), (Rr, Cc, 0, 3, D, 0, 0.0, 0), (Rr, Cc, 0, 2, 4, 0, 0.0, 0), (Rr, Cc, 0, 2, -1, 0, 0.0, 0),
             (Rr, Cc, 0, 2, D, 2, 0.0, 0), (Rr, Cc, 0, 2, D, 0, -1.0, 0), (Rr, Cc, 0, 2, D, 0, NAN, 0), (Rr, Cc, 0, 2, D, 0, INF, 1),
             (Rr, Cc, 0, 2, D, 0, 3.0, 5), (Rr, Cc, 0, 2, D, 0, 3.0, -1), (Rr, 4097, 0, 2, D, 0, 0.0, 0), (1 << 31, Cc, 0, 2, D, 0, 0.0, 0)]
    for fn in (lib.gridhip_contsub, lib.gridhip_contsub_dev):
        for (r, c, layout, ncomp, deg, mode, ns, ni) in cases:
            assert fn(None, r, c, layout, ncomp, deg, mode, px, pm, pd, pw, ns, ni, po, pc, pr, pcd, ps) == _lib.EINVAL
            assert fn(None, r, c, layout, ncomp, deg, mode, px, None, pd, None, ns, ni, po, None, None, None, None) == _lib.EINVAL
        assert fn(None, Rr, Cc, 0, 2, D, 0, None, pm, None, pw, 0.0, 0, None, pc, pr, pcd, ps) == _lib.EINVAL
        assert fn(None, Rr, Cc, 0, 2, D, 0, px, pm, pd, pw, 0.0, 0, pd, pd, pr, pcd, ps) == _lib.EINVAL   # coeffs over data
    for a, val in ((x, 0.5), (mk, 1), (data, 1 + 2j), (wt, 4.0), (out, 3 - 1j), (co, 7 + 0j), (ri, 5.0), (cd, 9), (st, 6.0)):
        assert np.all(a == val)


# ---- marshalling ---------------------------------------------------------------------------------------------------------
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


def test_contsub_marshalling(rig):
    ctx, rec, run = rig
    B, T, F = 2, 3, 5
    n = B * T * F
    vis = (np.arange(n) * (1 - 0.5j)).astype(c128).reshape(B, T, F)
    wt = np.arange(n, dtype=f64).reshape(B, T, F)
    x32 = np.linspace(-1, 1, F).astype(np.float32)           # converted: a small array
    mask = np.array([1, 1, 0, 1, 1], dtype=bool)             # reinterpreted as bytes
    # axis -1, complex: layout 0, ncomp 2, R = B T; the cube and its weights go by their own addresses
    o, c, i, s = Out(c128, n), Out(c128, B * T * 3), Out(f64, B * T * 4), Out(f64, 8)
    got = run(lambda: ctx.contsub(vis, x32, mask=mask, weights=wt, degree=2, nsigma=3, niter=2), "gridhip_contsub",
              B * T, F, 0, 2, 2, 0, Arr(x32, f64), Arr([1, 1, 0, 1, 1], u8), Same(vis), Same(wt), 3.0, 2, o, c, i, None, s)
    assert o.returned(got[0], (B, T, F)) and c.returned(got[1], (B, T, 3)) and i.returned(got[2], (B, T, 4))
    assert got[3] is None and s.returned(got[4], (8,))
    # axis 0, real: layout 1, ncomp 1, R = N N; the defaults are degree 1, mode subtract, no rounds; model mode is 1;
    # codes on request; no coeffs and no info: NULL
    cube = np.arange(F * 4 * 4, dtype=f64).reshape(F, 4, 4)
    x = np.linspace(-1, 1, F)
    o, c, i, s = Out(f64, F * 16), Out(f64, 2 * 16), Out(f64, 4 * 16), Out(f64, 8)
    got = run(lambda: ctx.contsub(cube, x, axis=0), "gridhip_contsub", 16, F, 1, 1, 1, 0, Same(x), None, Same(cube), None, 0.0, 0,
              o, c, i, None, s)
    assert o.returned(got[0], (F, 4, 4)) and c.returned(got[1], (2, 4, 4)) and i.returned(got[2], (4, 4, 4))
    o, k = Out(f64, F * 16), Out(u8, F * 16)
    got = run(lambda: ctx.contsub(cube, x, axis=0, degree=0, mode="model", coeffs=False, info=False, codes=True),
              "gridhip_contsub", 16, F, 1, 1, 0, 1, Same(x), None, Same(cube), None, 0.0, 0, o, None, None, k, Out(f64, 8))
    assert got[1] is None and got[2] is None and k.returned(got[3], (F, 4, 4))
    # complex along axis 0 and real along axis -1; a one-dimensional spectrum is one row either way
    cz = np.zeros((F, 7), dtype=c128)
    run(lambda: ctx.contsub(cz, x, axis=0, degree=3), "gridhip_contsub", 7, F, 1, 2, 3, 0, Same(x), None, Same(cz), None, 0.0, 0,
        Out(c128, F * 7), Out(c128, 4 * 7), Out(f64, 4 * 7), None, Out(f64, 8))
    rz = np.zeros((7, F))
    run(lambda: ctx.contsub(rz, x), "gridhip_contsub", 7, F, 0, 1, 1, 0, Same(x), None, Same(rz), None, 0.0, 0,
        Out(f64, F * 7), Out(f64, 2 * 7), Out(f64, 4 * 7), None, Out(f64, 8))
    one = np.zeros(F)
    for axis in (-1, 0):
        got = run(lambda: ctx.contsub(one, x, axis=axis), "gridhip_contsub", 1, F, 0 if axis else 1, 1, 1, 0, Same(x), None, Same(one),
                  None, 0.0, 0, Out(f64, F), Out(f64, 2), Out(f64, 4), None, Out(f64, 8))
        assert got[1].shape == (2,) and got[2].shape == (4,)
    # in place: out may be the data, and is what comes back
    got = run(lambda: ctx.contsub(vis, x, out=vis), "gridhip_contsub", B * T, F, 0, 2, 1, 0, Same(x), None, Same(vis), None, 0.0, 0,
              Same(vis), Out(c128, B * T * 2), Out(f64, B * T * 4), None, Out(f64, 8))
    assert got[0] is vis


def test_wrong_arguments_are_refused_before_any_call(rig):
    import torch
    ctx, rec, run = rig
    F = 5
    vis, x = np.zeros((2, 3, F), dtype=c128), np.linspace(-1, 1, F)
    bad = [dict(data=np.zeros((2, 3, F), dtype=np.complex64)), dict(data=np.zeros((2, 3, F), dtype=np.float32)),
           dict(data=np.zeros((2, 3, 2 * F), dtype=c128)[:, :, ::2]), dict(data=np.zeros((2, 0, F), dtype=c128)),
           dict(data=[[0.0] * F]), dict(data=np.zeros((2, 4097))), dict(x=None), dict(x=x[:-1]), dict(x=x.astype(c128)),
           dict(x=np.zeros((F, 1))), dict(x=torch.zeros(F, dtype=torch.float64)), dict(mask=np.ones(F - 1, dtype=bool)),
           dict(mask=np.ones(F)), dict(mask=np.ones((1, F), dtype=u8)), dict(weights=np.ones((3, 2, F))),
           dict(weights=np.ones((2, 3, F), dtype=np.float32)), dict(weights=np.ones((2, 3, 2 * F))[:, :, ::2]),
           dict(weights=torch.ones((2, 3, F), dtype=torch.float64)), dict(degree=-1), dict(degree=4), dict(axis=1), dict(axis=-2),
           dict(mode="residual"), dict(nsigma=-1.0), dict(nsigma=np.nan), dict(nsigma=np.inf), dict(niter=-1), dict(niter=5),
           dict(out=np.zeros((2, 3, F))), dict(out=np.zeros((3, 2, F), dtype=c128)),
           dict(out=np.zeros((2, 3, 2 * F), dtype=c128)[:, :, ::2]), dict(axis=0, x=x)]   # (axis 0: C = 2, x holds 5)
    for change in bad:
        with pytest.raises(ValueError):
            ctx.contsub(**{**dict(data=vis, x=x), **change})
    assert rec.calls == []


# ---- the helper ------------------------------------------------------------------------------------------------------------
def test_channel_coordinate():
    import gridhip
    f = np.array([1.30e9, 1.10e9, 1.15e9, 1.50e9])
    x = gridhip.channel_coordinate(f)
    mid, half = 0.5 * (1.10e9 + 1.50e9), 0.5 * (1.50e9 - 1.10e9)
    assert x.dtype == f64 and R.same_bits(x, (f - mid) / half) and x.min() == -1.0 and x.max() == 1.0
    assert gridhip.channel_coordinate([1.4e9]).tolist() == [0.0] and gridhip.channel_coordinate([2.0, 2.0, 2.0]).tolist() == [0.0] * 3
    assert gridhip.channel_coordinate(np.arange(5.0)).tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    with pytest.raises(ValueError):
        gridhip.channel_coordinate([])


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_the_table_is_the_recurrence():
    x = np.array([-1.0, -0.3, 0.0, 0.7, 1.0])
    T = R.chebyshev_table(x, 3)
    assert T.shape == (7, 5) and (T[0] == 1).all() and R.same_bits(T[1], x)
    assert R.same_bits(T[2], (2.0 * x) * x - 1.0) and R.same_bits(T[3], (2.0 * x) * T[2] - x)
    assert np.allclose(T, np.cos(np.arange(7)[:, None] * np.arccos(x)[None, :]), atol=1e-14)
    assert R.chebyshev_table(x, 0).shape == (1, 5)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_independent_solve(seed):
    """The restatement against numpy.linalg.lstsq on the weighted Chebyshev Vandermonde matrix of every row's participants:
    R = 200, C = 96, D = 3, uniform x, weights in [0.5, 2] with 10 % zeros, a mask hole of 8 channels.  The normal equations
    at this conditioning (the basis is near-orthogonal on a uniform grid) agree with the QR solve to about 2e-14 of the
    largest coefficient; the bound 1e-12 leaves a factor of 50 for other seeds, and a wrong definition misses by 1e-3."""
    rng = np.random.default_rng(seed)
    Rr, Cc, D = 200, 96, 3
    x = np.linspace(-1.0, 1.0, Cc)
    w = rng.uniform(0.5, 2.0, (Rr, Cc))
    w[rng.random((Rr, Cc)) < 0.1] = 0.0
    mask = np.ones(Cc, dtype=bool)
    mask[40:48] = False
    T = R.chebyshev_table(x, D)
    a = rng.normal(size=(Rr, D + 1)) + 1j * rng.normal(size=(Rr, D + 1))
    data = a @ T[:D + 1] + 0.05 * (rng.normal(size=(Rr, Cc)) + 1j * rng.normal(size=(Rr, Cc)))
    data[:, 40:48] += 10.0   # (a line in the hole: it must not matter)
    out, coeffs, info, codes, stats = R.contsub(data, x, mask, w, degree=D)
    assert (info[:, 0] == D).all() and (codes[:, 40:48] != 0).all() and stats[7] == (w == 0).sum()
    worst = 0.0
    for r in range(Rr):
        m = codes[r] == 0
        sw = np.sqrt(w[r, m])
        sol = np.linalg.lstsq(sw[:, None] * T[:D + 1, m].T, sw * data[r, m], rcond=None)[0]
        worst = max(worst, np.abs(sol - coeffs[r]).max() / np.abs(sol).max())
    print(f"seed {seed}: worst coefficient error relative to the row's largest coefficient {worst:.2e}")
    assert worst < 1e-12
    # the same for real data, and out = data - the continuum of those coefficients
    outr, cr, _, _, _ = R.contsub(np.ascontiguousarray(data.real), x, mask, w, degree=D)
    assert R.same_bits(cr, np.ascontiguousarray(coeffs.real)) and R.same_bits(outr, np.ascontiguousarray(out.real))
    model = R.contsub(data, x, mask, w, degree=D, mode="model")[0]
    assert R.same_bits(data - model, out) and np.abs(model - coeffs @ T[:D + 1]).max() < 1e-13


def test_fallback():
    """one participant: degree 0 and a_0 that value; two: degree 1; none: degree -1 and out == data bit for bit"""
    rng = np.random.default_rng(4)
    Cc = 12
    x = np.linspace(-1.0, 1.0, Cc)
    data = rng.normal(size=(4, Cc)) + 1j * rng.normal(size=(4, Cc))
    data[3, 5] = -0.0
    w = np.zeros((4, Cc))
    w[0, 7] = 1.0
    w[1, [2, 9]] = 1.5, 0.5
    w[2, :] = 1.0
    out, coeffs, info, codes, stats = R.contsub(data, x, None, w, degree=3)
    assert info[:, 0].tolist() == [0, 1, 3, -1] and info[:, 1].tolist() == [1, 2, Cc, 0]
    assert coeffs[0, 0] == data[0, 7] and (coeffs[0, 1:] == 0).all() and (coeffs[1, 2:] == 0).all() and (coeffs[3] == 0).all()
    assert out[0, 7] == 0 and np.abs(out[1, [2, 9]]).max() < 1e-15      # the line through two points passes through them
    assert R.same_bits(out[3], data[3]) and np.isnan(info[3, 3]) and stats.tolist() == [4, 1, 2, 1, 1 + 2 + Cc, 0, 0, 4 * Cc - 3 - Cc]
    # two participants at the SAME x: the second pivot is not good, degree 0, the weighted mean
    out, coeffs, info, codes, stats = R.contsub(data[:1], np.zeros(Cc), None, w[1:2], degree=2)
    assert info[0, 0] == 0 and abs(coeffs[0, 0] - (1.5 * data[0, 2] + 0.5 * data[0, 9]) / 2.0) < 1e-15


def test_classes_and_a_channel_without_a_coordinate():
    Cc = 10
    x = np.linspace(-1.0, 1.0, Cc)
    x[4] = NAN
    data = np.arange(2 * Cc, dtype=f64).reshape(2, Cc) + 0j
    w = np.ones((2, Cc))
    w[0, 0], w[0, 1], w[0, 2], w[0, 3] = 0.0, -1.0, NAN, INF
    data[1, 0], data[1, 1] = NAN, 1j * INF
    mask = np.ones(Cc, dtype=u8)
    mask[9] = 0
    w[0, 9], data[1, 9] = 0.0, NAN          # (the first class that applies)
    out, coeffs, info, codes, stats = R.contsub(data, x, mask, w, degree=1)
    assert codes[0].tolist() == [1, 1, 1, 1, 2, 0, 0, 0, 0, 1] and codes[1].tolist() == [3, 3, 0, 0, 2, 0, 0, 0, 0, 3]
    assert np.isnan(out[:, 4]).all() and np.isfinite(out[0, :4]).all() and np.isfinite(out[:, 5:9]).all()
    assert stats.tolist() == [2, 2, 0, 0, 4 + 6, 0, 3, 5] and (codes == 2).sum() + stats[4:].sum() == 2 * Cc


def test_clipping():
    """Rows of a degree-3 continuum plus noise 0.1 plus a line of height 5 over 8 channels the mask leaves in, nsigma = 3,
    niter = 4: every line sample is clipped, and at most 1 % of the others - at the row count of this test and at the one
    the GPU test runs (which then only compares bits)."""
    for Rr in (200, 129):
        data, x, line = R.clip_case(CLIP_SEED, R=Rr)
        out, coeffs, info, codes, stats = R.contsub(data, x, degree=3, nsigma=3.0, niter=4)
        clipped = codes >= 16
        rounds = np.bincount(codes.ravel(), minlength=20)[16:20].tolist()
        print(f"R = {Rr}: line samples clipped {clipped[line].sum()} of {line.sum()}, others {clipped[~line].sum()} of "
              f"{(~line).sum()}; per round {rounds}; stats {stats.tolist()}")
        assert clipped[line].all() and clipped[~line].mean() <= 0.01
        assert stats[5] == clipped.sum() and (info[:, 2] == clipped.sum(axis=1)).all() and (info[:, 0] == 3).all()
        # the continuum is recovered where the first fit was pulled up by the line
        first = R.contsub(data, x, degree=3)[0]
        assert np.abs(out[~line]).std() < 0.15 and np.abs(first[~line]).std() > 2 * np.abs(out[~line]).std()
    # nsigma == 0 skips the rounds whatever niter says
    assert R.same_bits(R.contsub(data, x, degree=3, nsigma=0.0, niter=4)[3], np.zeros(data.shape, dtype=u8))
