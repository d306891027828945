"""Rotation-measure synthesis and RM-CLEAN (gridhip_rm_tables, gridhip_rmsynth, gridhip_rmclean and their _dev forms,
gridhip_rm_tile), the checks that need no GPU: the library, the header, the ctypes table and both bindings carry the seven
entry points; a NULL context is refused; Context.rm_tables / rmsynth / rmclean hand the ABI the right pointers and refuse
wrong shapes and scalars before any call; faraday_grid against its formulas; and the numpy restatement the GPU tests compare
with (tests/rm_ref.py): the synthesis against a direct long-double sum, the RMSF's symmetry, RM-CLEAN on a J = 3 case worked
by hand and on two components that it must recover."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import rm_ref as R
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_rm_tables", "gridhip_rm_tables_dev", "gridhip_rmsynth", "gridhip_rmsynth_dev", "gridhip_rmclean",
         "gridhip_rmclean_dev", "gridhip_rm_tile"]
f64, c128 = np.float64, np.complex128
LAM2 = np.linspace(0.03, 0.09, 48)  # 48 channels: fwhm = 2 sqrt(3) / 0.06 = 57.7 rad / m^2


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_seven():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    for name in NAMES[:6:2]:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name + "_dev"]
    for macro, value in (("MAX_CHANNELS", 1024), ("MAX_DEPTHS", 512), ("HEAD", 16), ("MAPS", 7), ("STATS", 8)):
        assert re.search(rf"#define GRIDHIP_RM_{macro} {value}\b", raw), macro
    assert "#define GRIDHIP_RM_TABLE_DOUBLES(C, J) (16 + 2 * (C) * (J) + 3 * (2 * (J) - 1))" in raw


def test_header_states_the_semantics():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("rotation-measure synthesis"):raw.index("int gridhip_rm_tables(")]
    for phrase in ("Brentjens", "Heald", "LINE OF SIGHT", "0.3183098861837907", "t - rint(t)", "sincospi(2 r)", "lag_k",
                   "2.772588722239781", "acc.re = acc.re + (E.re * q - E.im * u)", "ties to the lowest j",
                   "a NaN never selected", "p_k <= L2", "reason 3", "not exactly", "phi_fit", "NaN sigma", "16-byte aligned",
                   "No floating-point atomic", "captured into a", "NOT HERE", "QU-fitting", "multi-scale"):
        assert phrase in section, phrase


def test_bindings_carry_the_seven():
    import gridhip
    for fn in (gridhip.Context.rm_tables, gridhip.Context.rmsynth, gridhip.Context.rmclean, gridhip.rm_tile, gridhip.faraday_grid):
        assert callable(fn)
    assert "rm_tile" in gridhip.__all__ and "faraday_grid" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
        assert name in doc, name


def test_the_tile():
    import gridhip
    from gridhip import _lib
    tm, tj, kc = gridhip.rm_tile()
    assert tm >= 1 and tj >= 1 and kc >= 1 and tm * tj >= 256
    assert _lib.load().gridhip_rm_tile(None) == _lib.EINVAL


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists: the argument rules themselves are checked on the GPU
    (test_gpu_rm.py::test_refusals); here a NULL context is GRIDHIP_EINVAL for good and bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    Cn, J, M = 2, 3, 4
    lam2, tab = np.full(Cn, 0.5), np.full(R.table_doubles(Cn, J), 7.0)
    q, u, cube = np.full((Cn, M), 1.0), np.full((Cn, M), 2.0), np.full((J, M), 3 + 4j)
    maps, st, noise = np.full((7, M), 5.0), np.full(8, 6.0), np.full(1, 0.5)
    pl, pt, pq, pu, pc, pm, ps, pn = (C.c_void_p(a.ctypes.data) for a in (lam2, tab, q, u, cube, maps, st, noise))
    for fn in (lib.gridhip_rm_tables, lib.gridhip_rm_tables_dev):
        assert fn(None, Cn, J, pl, None, -1.0, 1.0, 2.0, pt) == _lib.EINVAL
        assert fn(None, 0, J, pl, None, -1.0, 0.0, 2.0, None) == _lib.EINVAL
    for fn in (lib.gridhip_rmsynth, lib.gridhip_rmsynth_dev):
        assert fn(None, M, Cn, J, pt, pq, pu, pc, ps) == _lib.EINVAL
        assert fn(None, 0, Cn, 513, pt, None, pu, pc, ps) == _lib.EINVAL
    for fn in (lib.gridhip_rmclean, lib.gridhip_rmclean_dev):
        assert fn(None, M, J, pt, pc, None, 0.1, 0.0, 10, 0.0, None, 0, pm, ps) == _lib.EINVAL
        assert fn(None, M, J, pt, pc, None, np.nan, 0.0, -1, 3.0, pn, 1, pm, ps) == _lib.EINVAL
    for a, val in ((lam2, 0.5), (tab, 7.0), (q, 1.0), (u, 2.0), (cube, 3 + 4j), (maps, 5.0), (st, 6.0), (noise, 0.5)):
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


class One:
    """the argument addresses one double of this value"""

    def __init__(self, value):
        self.value = value

    def check(self, arg, where):
        assert np.frombuffer((C.c_char * 8).from_address(arg.value), dtype=f64)[0] == self.value, where


def test_marshalling(rig):
    ctx, rec, run = rig
    Cn, J, N = 3, 5, 4
    n = R.table_doubles(Cn, J)
    lam2 = np.array([0.01, 0.02, 0.04], dtype=np.float32)
    w = np.array([1, 2, 3])
    t = Out(f64, n)
    got = run(lambda: ctx.rm_tables(lam2, (-2.0, 1.0, J), weights=w, fwhm=3.0), "gridhip_rm_tables", Cn, J, Arr(lam2, f64),
              Arr(w, f64), -2.0, 1.0, 3.0, t)
    assert t.returned(got, (n,))
    l64 = lam2.astype(f64)
    run(lambda: ctx.rm_tables(l64, (-2.0, 1.0, J)), "gridhip_rm_tables", Cn, J, Same(l64), None, -2.0, 1.0,
        2.0 * math.sqrt(3.0) / float(l64[2] - l64[0]), Out(f64, n))
    # rmsynth: the images keep their shape; C from q, J from the table's length
    tab = np.zeros(n)
    q = np.arange(Cn * N * N, dtype=np.float32).reshape(Cn, N, N)
    u = np.arange(2 * Cn * N * N, dtype=f64)[::2].reshape(Cn, N, N)
    cube, st = Out(c128, J * N * N), Out(f64, 8)
    got = run(lambda: ctx.rmsynth(q, u, tab), "gridhip_rmsynth", N * N, Cn, J, Same(tab), Arr(q, f64), Arr(u, f64), cube, st)
    assert cube.returned(got[0], (J, N, N)) and st.returned(got[1], (8,))
    out = np.zeros((J, 7), dtype=c128)
    got = run(lambda: ctx.rmsynth(q.reshape(Cn, -1)[:, :7], u.reshape(Cn, -1)[:, :7], tab, out=out), "gridhip_rmsynth", 7, Cn, J,
              Same(tab), Arr(q.reshape(Cn, -1)[:, :7], f64), Arr(u.reshape(Cn, -1)[:, :7], f64), Same(out), Out(f64, 8))
    assert got[0] is out
    # rmclean: the cube in place, a new model of zeros, the defaults, NULL noise
    cb = np.ones((J, N, N), dtype=c128)
    model, maps = Arr(np.zeros(J * N * N), c128), Out(f64, 7 * N * N)
    got = run(lambda: ctx.rmclean(cb, tab), "gridhip_rmclean", N * N, J, Same(tab), Same(cb), model, 0.1, 0.0, 100, 0.0, None, 0,
              maps, Out(f64, 8))
    assert got[1] is cb and got[0].shape == (J, N, N) and got[0].dtype == c128 and maps.returned(got[2], (7, N, N))
    md, noise = np.zeros((J, N, N), dtype=c128), np.array([0.25])
    got = run(lambda: ctx.rmclean(cb, tab, gain=0.2, threshold=0.5, niter=7, nsigma=3, noise=noise, restore=True, model=md),
              "gridhip_rmclean", N * N, J, Same(tab), Same(cb), Same(md), 0.2, 0.5, 7, 3.0, Same(noise), 1, Out(f64, 7 * N * N),
              Out(f64, 8))
    assert got[0] is md
    run(lambda: ctx.rmclean(cb, tab, nsigma=2, noise=0.5), "gridhip_rmclean", N * N, J, Same(tab), Same(cb),
        Arr(np.zeros(J * N * N), c128), 0.1, 0.0, 100, 2.0, One(0.5), 0, Out(f64, 7 * N * N), Out(f64, 8))


def test_wrong_shapes_and_scalars_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    Cn, J, M = 3, 5, 6
    lam2, tab = np.array([0.01, 0.02, 0.04]), np.zeros(R.table_doubles(Cn, J))
    q, u, cube = np.zeros((Cn, M)), np.zeros((Cn, M)), np.zeros((J, M), dtype=c128)
    for kw in (dict(lam2=np.zeros((2, 2))), dict(lam2=np.zeros(0)), dict(lam2=np.zeros(1025)), dict(phi=(0.0, 1.0)),
               dict(phi=(0.0, 0.0, J)), dict(phi=(0.0, -1.0, J)), dict(phi=(np.nan, 1.0, J)), dict(phi=(0.0, 1.0, 0)),
               dict(phi=(0.0, 1.0, 513)), dict(weights=np.ones(2)), dict(weights=np.ones(Cn, dtype=c128)), dict(fwhm=0.0),
               dict(fwhm=np.inf), dict(lam2=np.full(Cn, 0.5)), dict(lam2=lam2.astype(c128))):
        with pytest.raises(ValueError):
            ctx.rm_tables(**{**dict(lam2=lam2, phi=(-2.0, 1.0, J)), **kw})
    for kw in (dict(q=np.zeros(M)), dict(u=np.zeros((Cn, M + 1))), dict(q=np.zeros((Cn, 0)), u=np.zeros((Cn, 0))),
               dict(q=q.astype(c128)), dict(tables=tab[:-1]), dict(tables=tab.astype(np.float32)), dict(tables=None),
               dict(tables=np.zeros(R.table_doubles(Cn + 1, J))), dict(out=np.zeros((J, M))), dict(out=np.zeros((J + 1, M), dtype=c128)),
               dict(u=None)):
        with pytest.raises(ValueError):
            ctx.rmsynth(**{**dict(q=q, u=u, tables=tab), **kw})
    for kw in (dict(cube=np.zeros((J, M))), dict(cube=np.zeros(J, dtype=c128)), dict(cube=np.zeros((J, 2 * M), dtype=c128)[:, ::2]),
               dict(cube=np.zeros((J + 2, M), dtype=c128)), dict(cube=np.zeros((513, M), dtype=c128)), dict(gain=np.nan),
               dict(threshold=np.inf), dict(niter=-1), dict(nsigma=-1.0), dict(nsigma=np.inf), dict(nsigma=2.0),
               dict(nsigma=2.0, noise=np.zeros(2)), dict(noise=np.zeros(1, dtype=np.float32)), dict(model=np.zeros((J, M))),
               dict(model=np.zeros((J, M + 1), dtype=c128)), dict(tables=tab[1:])):
        with pytest.raises(ValueError):
            ctx.rmclean(**{**dict(cube=cube, tables=tab), **kw})
    assert rec.calls == []


# ---- faraday_grid ----------------------------------------------------------------------------------------------------------
def test_faraday_grid_against_its_formulas():
    import gridhip
    lam2 = [0.03, 0.01, 0.04, 0.02]  # (any order)
    phi0, dphi, J, fwhm, max_scale, phi_limit = gridhip.faraday_grid(lam2)
    s = sorted(lam2)
    assert fwhm == 2.0 * math.sqrt(3.0) / (s[3] - s[0]) and dphi == fwhm / 4.0
    assert phi_limit == math.sqrt(3.0) / max(abs(b - a) for a, b in zip(s, s[1:]))
    assert max_scale == math.pi / 0.01
    # (phi_limit / dphi is 6 but for the rounding of the channel gaps: either side of it is the formula's floor)
    assert J in (2 * math.floor(phi_limit / dphi * (1 - 1e-12)) + 1, 2 * math.floor(phi_limit / dphi * (1 + 1e-12)) + 1)
    assert J % 2 == 1 and phi0 == -(J - 1) / 2 * dphi and phi0 + (J - 1) // 2 * dphi == 0.0
    g = gridhip.faraday_grid(lam2, oversample=8, phi_max=100.0)
    assert g[1] == fwhm / 8.0 and g[2] == 2 * math.floor(100.0 / g[1]) + 1 and g[3:] == (fwhm, max_scale, phi_limit)
    assert gridhip.faraday_grid(lam2, oversample=64, phi_max=1e6)[2] == 511
    for bad in (dict(lam2=[0.01]), dict(lam2=[0.01, 0.01]), dict(lam2=[0.01, np.nan]), dict(lam2=[0.0, 0.01]),
                dict(lam2=lam2, oversample=0), dict(lam2=lam2, phi_max=-1.0)):
        with pytest.raises(ValueError):
            gridhip.faraday_grid(**bad)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def grid48():
    fwhm = 2.0 * math.sqrt(3.0) / (LAM2[-1] - LAM2[0])
    dphi, J = fwhm / 4.0, 65
    return -(J - 1) / 2 * dphi, dphi, J, fwhm


def test_tables_restatement_within_its_own_bounds_and_the_rmsf_is_hermitian():
    phi0, dphi, J, fwhm = grid48()
    w = np.linspace(0.5, 1.5, 48)
    tab = R.tables(LAM2, w, phi0, dphi, J, fwhm)
    R.check_tables(tab, LAM2, w, phi0, dphi, J, fwhm)
    head, E, Rm, G = R.parts(tab, 48, J)
    assert head[0] == 1.0 and abs(Rm[J - 1].real - 1.0) <= 48 * R.U and Rm[J - 1].imag == 0.0
    assert np.abs(Rm[::-1] - np.conj(Rm)).max() <= 1e-14  # R[-k] = conj R[k]
    assert np.all(np.abs(Rm) <= 1.0 + 1e-14) and G[J - 1] == 1.0 and np.array_equal(G, G[::-1])
    # the width of |R| at half its height is the fwhm the formula promises, to a depth step
    half = np.flatnonzero(np.abs(Rm) >= 0.5)
    assert abs((half[-1] - half[0] + 1) * dphi - fwhm) <= 2.0 * dphi
    for lam2, wt in (([0.1, np.nan], None), ([0.1, 0.2], [1.0, -1.0]), ([0.1, 0.2], [0.0, 0.0]), ([0.1, np.inf], None)):
        bad = R.tables(lam2, wt, phi0, dphi, 3, fwhm)
        assert bad[0] == 0.0 and not np.any(bad[R.HEAD:] != 0.0) and bad[1] == 2 and bad[2] == 3
        R.check_tables(bad, lam2, wt, phi0, dphi, 3, fwhm)


def test_synth_against_a_direct_long_double_sum():
    phi0, dphi, J, fwhm = grid48()
    rng = np.random.default_rng(5)
    tab = R.tables(LAM2, None, phi0, dphi, J, fwhm)
    Q, U, _ = R.sky(rng, LAM2, phi0, dphi, J, 9)
    cube, stats = R.synth(tab, Q, U)
    ld = np.longdouble
    a = LAM2.astype(ld) - ld(tab[5])
    phi = ld(phi0) + np.arange(J).astype(ld) * ld(dphi)
    ang = -2 * phi[:, None] * a[None, :]
    Er, Ei = np.cos(ang) / 48, np.sin(ang) / 48  # [J][C]
    ref_re = Er @ Q.astype(ld) - Ei @ U.astype(ld)
    ref_im = Er @ U.astype(ld) + Ei @ Q.astype(ld)
    scale = (np.abs(Q) + np.abs(U)).sum(axis=0) / 48
    err = np.maximum(np.abs(cube.real - ref_re.astype(f64)), np.abs(cube.imag - ref_im.astype(f64)))
    assert np.all(err <= 1e-12 * scale[None, :]) and not stats.any()
    # a bad line of sight is NaN at every depth and counted; its neighbours are as they were
    Q2, U2 = Q.copy(), U.copy()
    Q2[7, 3], U2[0, 5] = np.nan, np.inf
    c2, s2 = R.synth(tab, Q2, U2)
    good = [0, 1, 2, 4, 6, 7, 8]
    assert np.isnan(c2[:, [3, 5]]).all() and np.array_equal(c2[:, good], cube[:, good]) and s2[0] == 2 and not s2[1:].any()
    none, s3 = R.synth(R.tables([0.1, np.nan], None, phi0, dphi, J, fwhm), Q[:2], U[:2])
    assert none is None and s3[7] == 1 and not s3[:7].any()
    none, s3 = R.synth(tab, Q[:47], U[:47])  # another C
    assert none is None and s3[7] == 1
    # one Faraday-thin source on a grid depth: the peak is there and |F| is its amplitude
    P = (0.7 * np.exp(0.6j)) * np.exp(2j * (phi0 + 40 * dphi) * LAM2)
    one, _ = R.synth(tab, P.real[:, None], P.imag[:, None])
    assert np.argmax(np.abs(one[:, 0])) == 40 and abs(abs(one[40, 0]) - 0.7) <= 1e-12


def hand_table():
    """C = 1, J = 3, phi = -1, 0, 1; R = G = (0, 0.5, 1, 0.5, 0) at the lags -2 .. 2"""
    tab = np.zeros(R.table_doubles(1, 3))
    tab[:9] = [1, 1, 3, -1.0, 1.0, 0.5, 1.0, 1.0, 2.0]
    tab[16:22:2] = 1.0  # E
    tab[22:32:2] = [0, 0.5, 1, 0.5, 0]
    tab[32:37] = [0, 0.5, 1, 0.5, 0]
    return tab


def test_rmclean_on_a_case_worked_by_hand():
    """F = (0, 4, 1), gain 0.5, level 1.  The components: k = 1, f = 2 -> (-1, 2, 0); k = 1, f = 1 -> (-1.5, 1, -0.5);
    k = 0, f = -0.75 -> (-0.75, 1.375, -0.5); k = 1, f = 0.6875 -> (-1.09375, 0.6875, -0.84375); k = 0, f = -0.546875 ->
    (-0.546875, 0.9609375, -0.84375), whose largest p = 0.9234 <= 1: reason 1 after 5 components.  Every number is dyadic."""
    tab = hand_table()
    cube = np.array([[0.0], [4.0], [1.0]], dtype=c128)
    model, res, maps, stats, gap = R.rmclean(tab, cube, gain=0.5, threshold=1.0, niter=10)
    assert np.array_equal(res[:, 0], [-0.546875, 0.9609375, -0.84375]) and np.array_equal(model[:, 0], [-1.296875, 3.6875, 0.0])
    ps, pm, pp = 0.9609375 ** 2, 0.546875 ** 2, 0.84375 ** 2
    fit = 0.0 + ((0.5 * (pm - pp)) / ((pm - ps) + (pp - ps))) * 1.0
    assert np.array_equal(maps[:, 0], [5, 1, 1, ps, fit, 0.9609375, 0.0])
    assert np.array_equal(stats, [0, 5, 0, 1, 0, 1.0, 0, 0]) and 0 < gap < 1
    # niter first: three components, then the level is still exceeded
    model, res, maps, stats, _ = R.rmclean(tab, cube, gain=0.5, threshold=1.0, niter=3)
    assert np.array_equal(res[:, 0], [-0.75, 1.375, -0.5]) and np.array_equal(maps[:3, 0], [3, 0, 1]) and stats[2] == 1
    # niter = 0 takes nothing; a level above the peak stops at once with reason 1
    model, res, maps, stats, _ = R.rmclean(tab, cube, niter=0)
    assert np.array_equal(res, cube) and not model.any() and np.array_equal(maps[:4, 0], [0, 0, 1, 16.0])
    model, res, maps, stats, _ = R.rmclean(tab, cube, threshold=4.0)
    assert np.array_equal(res, cube) and np.array_equal(maps[:2, 0], [0, 1])
    # G = R here: the restore puts back what was taken, on top of a model carried in
    model, res, maps, stats, _ = R.rmclean(tab, cube, gain=0.5, threshold=1.0, niter=10, restore=True)
    assert np.array_equal(res[:, 0], [0.0, 4.0, 1.0]) and np.array_equal(maps[:4, 0], [5, 1, 1, 16.0])
    carried = np.array([[0.0], [0.0], [2.0]], dtype=c128)
    model, res, _, _, _ = R.rmclean(tab, cube, model=carried, gain=0.5, threshold=1.0, niter=10, restore=True)
    assert np.array_equal(model[:, 0], [-1.296875, 3.6875, 2.0]) and np.array_equal(res[:, 0], [0.0, 5.0, 3.0])
    # the level from the noise; a NaN sigma and a table that does not fit touch nothing
    _, _, _, stats, _ = R.rmclean(tab, cube, gain=0.5, threshold=0.5, nsigma=4.0, noise=np.array([0.25]), niter=10)
    assert stats[5] == 1.0 and stats[1] == 5
    model, res, maps, stats, _ = R.rmclean(tab, cube, nsigma=1.0, noise=np.array([np.nan]))
    assert maps is None and np.array_equal(stats, [0, 0, 0, 0, 0, 0, 1, 0]) and np.array_equal(res, cube)
    bad = tab.copy()
    bad[0] = 0.0
    model, res, maps, stats, _ = R.rmclean(bad, cube)
    assert maps is None and np.array_equal(stats, [0, 0, 0, 0, 0, 0, 0, 1]) and np.array_equal(res, cube)
    # a line of sight with a NaN is left alone; a tie goes to the lowest depth
    two = np.array([[0.0, 3.0], [np.nan, -3.0], [1.0, 3.0j]], dtype=c128)
    model, res, maps, stats, _ = R.rmclean(tab, two, gain=0.5, threshold=1.0, niter=1)
    assert np.isnan(res[1, 0]) and res[0, 0] == 0 and res[2, 0] == 1 and np.array_equal(maps[:3, 0], [0, 3, -1])
    assert np.isnan(maps[3:, 0]).all() and stats[0] == 1 and model[0, 1] == 1.5 and not model[1:, 1].any()


def test_two_components_are_recovered():
    """Two Faraday-thin sources 20 depth steps = 5 FWHM apart, no noise: cleaned to the level L and restored, the two
    peaks are at their depths (within dphi: on them) and of their amplitudes within L."""
    phi0, dphi, J, fwhm = grid48()
    tab = R.tables(LAM2, None, phi0, dphi, J, fwhm)
    amps = {20: 1.0 * np.exp(0.3j), 40: 0.6 * np.exp(-1.1j)}
    P = sum(a * np.exp(2j * (phi0 + j * dphi) * LAM2) for j, a in amps.items())
    cube, _ = R.synth(tab, P.real[:, None], P.imag[:, None])
    L = 0.01
    model, rest, maps, stats, gap = R.rmclean(tab, cube, gain=0.1, threshold=L, niter=1000, restore=True)
    assert maps[1, 0] == 1 and stats[3] == 1 and gap > 1e-9
    mag = np.abs(rest[:, 0])
    peaks = [j for j in range(1, J - 1) if mag[j] > mag[j - 1] and mag[j] > mag[j + 1] and mag[j] > 0.3]
    assert peaks == [20, 40]
    for j, a in amps.items():
        assert abs(mag[j] - abs(a)) <= L, (j, mag[j])
    assert maps[2, 0] == 20 and abs(maps[4, 0] - (phi0 + 20 * dphi)) <= dphi
