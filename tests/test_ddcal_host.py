"""Direction-dependent calibration (gridhip_ddcal*, gridhip_dd_subtract*, gridhip_imager_peel_dev,
gridhip_ddcal_lds_antennas), the checks that need no GPU: the library, the header, the ctypes table, both bindings and the
hpp carry the entry points; a NULL context or imager is refused with GRIDHIP_EINVAL whatever else is passed;
Context.ddcal and Context.dd_subtract hand the ABI the right pointers, scalar order and NULLs (against the recording
library of test_binding_marshalling.py); the LDS limit is the header's formula; and the numpy restatement the GPU tests
compare with (tests/ddcal_ref.py) is right on worked cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddcal_ref as R
import gaincal_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same
from test_gaincal_host import corrupted

NAMES = ["gridhip_ddcal", "gridhip_ddcal_dev", "gridhip_dd_subtract", "gridhip_dd_subtract_dev", "gridhip_imager_peel_dev",
         "gridhip_ddcal_lds_antennas"]
f64, c128, i64 = np.float64, np.complex128, np.int64


def dd_case(rng, A, T, D, reps=3, noise=0.0, weights=False):
    """Every baseline of A antennas, `reps` dumps per interval, D point-source models at random positions, gains
    1 + 0.3 (N + iN): -> a1, a2, slot, V, M [D][n], w, the true gains [D][T][A]"""
    p, q = np.triu_indices(A, 1)
    a1, a2 = np.tile(p, T * reps), np.tile(q, T * reps)
    sl = np.repeat(np.arange(T), len(p) * reps)
    n = len(a1)
    u, v = rng.uniform(-300, 300, n), rng.uniform(-300, 300, n)
    l, m = rng.uniform(-0.05, 0.05, D), rng.uniform(-0.05, 0.05, D)
    M = np.exp(-2j * np.pi * (u[None] * l[:, None] + v[None] * m[:, None])) * rng.uniform(1, 3, D)[:, None]
    gt = 1 + 0.3 * (rng.normal(size=(D, T, A)) + 1j * rng.normal(size=(D, T, A)))
    V = R.model_sum(gt, a1, a2, sl, M) + noise * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return a1, a2, sl, V, M, (rng.uniform(0.5, 2, n) if weights else np.ones(n)), gt


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_entry_points():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\b(int|int64_t) {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_ddcal"] == _lib.SIGNATURES["gridhip_ddcal_dev"]
    assert _lib.SIGNATURES["gridhip_dd_subtract"] == _lib.SIGNATURES["gridhip_dd_subtract_dev"]
    # gaincal's arguments with D after T
    gc = _lib.SIGNATURES["gridhip_gaincal"][1]
    assert _lib.SIGNATURES["gridhip_ddcal"][1] == gc[:4] + [_lib.i64] + gc[4:]
    assert _lib.load().gridhip_version() >= 260
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 260
    section = raw[raw.index("direction-dependent calibration"):raw.index("int gridhip_ddcal(")]
    for phrase in ("GRIDHIP_EUNSUPPORTED", "2^21", "DETERMINISM", "FLAGGED", "DROPPED", "AUTO", "UNSOLVED", "SOLVED", "LDL^H",
                   "1e-12", "LDS BUDGET", "131072", "NOT bit for bit"):
        assert phrase in section, phrase


def test_bindings_carry_the_entry_points():
    import gridhip
    for owner, method in ((gridhip.Context, "ddcal"), (gridhip.Context, "dd_subtract"), (gridhip.Imager, "peel"),
                          (gridhip, "ddcal_lds_antennas")):
        assert callable(getattr(owner, method)), method
    assert "ddcal_lds_antennas" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("ddcalIO", "ddSubtractIO", "imagerPeelIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bddcal\s*\(", hpp) and re.search(r"\bdd_subtract\s*\(", hpp)
    for name in NAMES:
        assert name in hpp, name


def test_lds_antennas_is_the_headers_formula():
    import gridhip
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    budget = int(re.search(r"gridhip_ddcal_lds_antennas\(D\) = floor\((\d+) / \(\(D\^2 \+ 4 D\) \* 8\)\)", raw).group(1))
    assert budget == 128 * 1024 and budget <= 160 * 1024
    lib = _lib.load()
    for D in range(1, 9):
        want = budget // ((D * D + 4 * D) * 8)
        assert lib.gridhip_ddcal_lds_antennas(D) == want == gridhip.ddcal_lds_antennas(D), D
    assert gridhip.ddcal_lds_antennas(4) == 512
    for D in (0, -1, 9, 1 << 40):
        assert lib.gridhip_ddcal_lds_antennas(D) == 0, D  # the header: 0 for D outside 1..8


def test_null_handles_are_refused_and_nothing_is_touched():
    from gridhip import _lib
    lib = _lib.load()
    n, A, T, D = 3, 3, 1, 2
    a1, a2, sl = np.array([0, 0, 1], dtype=i64), np.array([1, 2, 2], dtype=i64), np.zeros(n, dtype=i64)
    vis, mod, out = np.full(n, 1 + 2j), np.full((D, n), 3 + 0j), np.full(n, 7 + 7j)
    wt, wo, g, st = np.full(n, 4.0), np.full(n, 8.0), np.full((D, T, A), 5 + 5j), np.full(8, 6.0)
    model = np.full((4, 4), 2.0)
    p1, p2, ps, pv, pm, po, pw, pwo, pg, pst, pmod = (C.c_void_p(a.ctypes.data)
                                                      for a in (a1, a2, sl, vis, mod, out, wt, wo, g, st, model))
    for fn in (lib.gridhip_ddcal, lib.gridhip_ddcal_dev):
        for (nn, AA, TT, DD, slot, mode, ref, niter, tol) in [
                (n, A, T, D, ps, 0, 0, 5, 1e-8), (n, A, T, 1, None, 1, -1, 0, 0.0), (-1, A, T, D, ps, 0, 0, 5, 0.0),
                (n, 1, T, D, ps, 0, 0, 5, 0.0), (n, A, 0, D, ps, 0, 0, 5, 0.0), (n, A, T, 0, ps, 0, 0, 5, 0.0),
                (n, A, T, 9, ps, 0, 0, 5, 0.0), (n, A, T, D, ps, 2, 0, 5, 0.0), (n, A, T, D, ps, 0, A, 5, 0.0),
                (n, A, T, D, ps, 0, 0, -1, 0.0), (n, A, T, D, ps, 0, 0, 5, float("nan")), (n, 1 << 10, 1 << 10, 4, ps, 0, 0, 1, 0.0)]:
            assert fn(None, nn, AA, TT, DD, p1, p2, slot, pv, pm, pw, mode, ref, 0, niter, tol, pg, pst) == _lib.EINVAL
            assert fn(None, nn, AA, TT, DD, p1, p2, slot, pv, pm, None, mode, ref, 1, niter, tol, pg, None) == _lib.EINVAL
        assert fn(None, n, A, T, D, p1, p2, ps, pv, pm, pw, 0, 0, 0, 5, 0.0, pm, pst) == _lib.EINVAL  # gains over model_vis
    for fn in (lib.gridhip_dd_subtract, lib.gridhip_dd_subtract_dev):
        for dirs in (0, 1, 3, 4, -1):
            assert fn(None, n, A, T, D, p1, p2, ps, pg, pm, dirs, pv, po) == _lib.EINVAL
            assert fn(None, n, A, T, D, p1, p2, None, pg, pm, dirs, None, pv) == _lib.EINVAL
        assert fn(None, n, A, T, D, p1, p2, ps, pg, pm, 3, pv, pg) == _lib.EINVAL  # vis_out over gains
    for mode in (0, 1, 5):
        assert lib.gridhip_imager_peel_dev(None, pmod, pv, A, T, D, p1, p2, ps, pw, mode, 0, 0, 5, 1e-8, pm, pg, po, pwo,
                                           pst) == _lib.EINVAL
        assert lib.gridhip_imager_peel_dev(None, None, None, 1, 0, 0, None, None, None, None, mode, 9, 0, -1, -1.0, None,
                                           None, None, None, None) == _lib.EINVAL
    for a, val in ((vis, 1 + 2j), (mod, 3 + 0j), (out, 7 + 7j), (wt, 4.0), (wo, 8.0), (g, 5 + 5j), (st, 6.0), (model, 2.0)):
        assert np.all(a == val)


# ---- marshalling ----------------------------------------------------------------------------------------------------------
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


def awkward():
    vis = (np.arange(2 * N) * (1 - 0.5j)).astype(c128)[::2]  # not contiguous
    mod = (np.arange(3 * N).reshape(3, N) + 1j).astype(np.complex64)
    return vis, mod


def test_ddcal_marshalling(rig):
    ctx, rec, run = rig
    vis, mod = awkward()
    wt = np.arange(N, dtype=np.float32)
    g_out, st_out = Out(c128, 3 * 2 * 3), Out(f64, 8)
    g, st = run(lambda: ctx.ddcal(vis, mod, A1, A2, 3, slot=SLOT, nslots=2, weights=wt, phase_only=True, refant=None,
                                  niter=7, tol=1e-6),
                "gridhip_ddcal", N, 3, 2, 3, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(vis, c128), Arr(mod, c128),
                Arr(wt, f64), 1, -1, 0, 7, 1e-6, g_out, st_out)
    assert g_out.returned(g, (3, 2, 3)) and st_out.returned(st, (8,))
    # a one-dimensional model is one direction; arrays in the ABI's form go by their own address; gains: the warm start
    v2, m2 = np.ascontiguousarray(vis), np.ascontiguousarray(mod[0], dtype=c128)
    a1, a2 = np.array(A1, dtype=i64), np.array(A2, dtype=i64)
    warm = np.ones((1, 1, 3), dtype=c128)
    g, st = run(lambda: ctx.ddcal(v2, m2, a1, a2, 3, gains=warm),
                "gridhip_ddcal", N, 3, 1, 1, Same(a1), Same(a2), None, Same(v2), Same(m2), None, 0, 0, 1, 50, 1e-8,
                Same(warm), Out(f64, 8))
    assert g is warm


def test_dd_subtract_marshalling(rig):
    ctx, rec, run = rig
    vis, mod = awkward()
    gains = (np.arange(18).reshape(3, 2, 3) + 2j).astype(np.complex64)
    o = Out(c128, N)
    out = run(lambda: ctx.dd_subtract(gains, mod, A1, A2, slot=SLOT, directions=[2, 0], vis=vis),
              "gridhip_dd_subtract", N, 3, 2, 3, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(gains, c128),
              Arr(mod, c128), 5, Arr(vis, c128), o)
    assert o.returned(out, (N,))
    # every direction, no input (the corrupted model itself), one interval, in the ABI's form, into the caller's array
    g1, m2, mine = np.ones((3, 1, 3), dtype=c128), np.ascontiguousarray(mod, dtype=c128), np.zeros(N, dtype=c128)
    out = run(lambda: ctx.dd_subtract(g1, m2, A1, A2, out=mine),
              "gridhip_dd_subtract", N, 3, 1, 3, Arr(A1, i64), Arr(A2, i64), None, Same(g1), Same(m2), 7, None, Same(mine))
    assert out is mine
    v2 = np.ascontiguousarray(vis)
    out = run(lambda: ctx.dd_subtract(g1, m2, A1, A2, directions=[], vis=v2, out=v2),
              "gridhip_dd_subtract", N, 3, 1, 3, Arr(A1, i64), Arr(A2, i64), None, Same(g1), Same(m2), 0, Same(v2), Same(v2))
    assert out is v2


def test_wrong_dtypes_and_shapes_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    vis, mod = awkward()
    ok = dict(vis=vis, model_vis=mod, a1=A1, a2=A2, nant=3)
    bad = [dict(model_vis=mod[:, :-1]), dict(model_vis=np.zeros((9, N), dtype=c128)), dict(model_vis=np.zeros((0, N), dtype=c128)),
           dict(model_vis=np.zeros((2, 3, N), dtype=c128)), dict(model_vis=None), dict(a1=np.array(A1, dtype=f64)),
           dict(nslots=2), dict(nant=1), dict(weights=np.ones(N - 1)), dict(gains=np.ones((1, 3), dtype=c128)),
           dict(gains=np.ones((3, 1, 3), dtype=np.complex64)), dict(gains=np.ones((2, 1, 3), dtype=c128)), dict(refant=3),
           dict(niter=-1), dict(tol=-1.0), dict(tol=float("nan"))]
    for change in bad:
        with pytest.raises(ValueError):
            ctx.ddcal(**{**ok, **change})
    g = np.ones((3, 2, 3), dtype=c128)
    for kw in [dict(gains=np.ones((2, 3), dtype=c128)), dict(gains=np.ones((2, 2, 3), dtype=c128)), dict(directions=[3]),
               dict(directions=[-1]), dict(slot=None), dict(out=np.zeros(N, dtype=np.complex64)), dict(vis=vis[:-1]),
               dict(out=np.zeros(N + 1, dtype=c128)), dict(a2=A2[:-1])]:
        args = {**dict(gains=g, model_vis=mod, a1=A1, a2=A2, slot=SLOT), **kw}
        with pytest.raises(ValueError):
            ctx.dd_subtract(args.pop("gains"), args.pop("model_vis"), args.pop("a1"), args.pop("a2"), **args)
    assert rec.calls == []


# ---- the numpy restatement on worked cases ---------------------------------------------------------------------------------
def test_one_direction_is_gaincal():
    a1, a2, sl, V, M, w, _ = corrupted(np.random.default_rng(21), 7, 3, noise=0.05)
    for mode in (0, 1):
        g, st, worst = R.ddcal(V, M[None], a1, a2, 7, slot=sl, T=3, wt=w, mode=mode, refant=3, niter=9, tol=0)
        g0, st0 = gaincal_ref.gaincal(V, M, a1, a2, 7, slot=sl, T=3, wt=w, mode=mode, refant=3, niter=9, tol=0)
        assert g.shape == (1, 3, 7) and np.abs(g[0] - g0).max() <= 1e-13 * np.abs(g0).max()
        assert np.array_equal(st[[0, 4, 5, 6, 7]], st0[[0, 4, 5, 6, 7]]) and np.allclose(st[1:4], st0[1:4], rtol=1e-12)
        assert worst == 1.0  # (one direction: the only pivot is H itself)


def test_the_true_gains_are_a_fixed_point_of_consistent_data():
    a1, a2, sl, V, M, w, gt = dd_case(np.random.default_rng(22), 6, 2, 3, weights=True)
    g, st, worst = R.ddcal(V, M, a1, a2, 6, slot=sl, T=2, wt=w, refant=-1, gains=gt, niter=3, tol=0)
    assert st[1] <= 1e-13 and np.abs(g - gt).max() <= 1e-13 and worst > 1e-6 and st[7] == 0


def test_one_baseline_two_directions_is_unsolved_everywhere():
    """A single visibility gives each antenna a rank-one H: the second pivot is zero up to rounding, nothing is solved and
    every gain keeps its bits."""
    warm = np.array([[[1 + 1j, 2 - 1j]], [[0.5j, 3 + 0j]]])
    piv = []
    g, st, worst = R.ddcal([2 + 1j], [[1 - 1j], [0.5 + 2j]], [0], [1], 2, gains=warm, niter=3, tol=0, pivots=piv)
    assert np.array_equal(g, warm) and st[7] == 2 and st[0] == 3 and st[1] == 0 and st[4] == 1
    assert worst < 1e-14 and all(r == 1.0 or abs(r) < 1e-14 for r in piv)


def test_a_zero_model_row_unsolves_exactly_those_antennas():
    a1, a2, sl, V, M, w, gt = dd_case(np.random.default_rng(23), 6, 1, 2)
    M = M.copy()
    M[1, (a1 == 4) | (a2 == 4)] = 0  # direction 1 has no model on any baseline of antenna 4
    V = R.model_sum(gt, a1, a2, sl, M)
    piv = []
    g, st, _ = R.ddcal(V, M, a1, a2, 6, refant=0, niter=6, tol=0, pivots=piv)
    assert st[7] == 1 and np.all(g[:, 0, 4] == 1) and not np.any(g[:, 0, [0, 1, 2, 3, 5]] == 1)
    assert all(r > 1e-6 or r == 0.0 for r in piv) and 0.0 in piv


@pytest.mark.parametrize("A,T,D", [(5, 1, 2), (6, 2, 2), (8, 2, 3), (10, 1, 4), (12, 2, 4), (16, 1, 3)])
def test_noise_free_recovery_of_known_gains(A, T, D):
    a1, a2, sl, V, M, _, gt = dd_case(np.random.default_rng(100 * A + 10 * T + D), A, T, D)
    g, st, worst = R.ddcal(V, M, a1, a2, A, slot=sl, T=T, refant=0, niter=200, tol=1e-10)
    truth = gt * np.exp(-1j * np.angle(gt[:, :, :1]))
    err = np.abs(g - truth).max()
    print(f"A={A} T={T} D={D}: {int(st[0])} iterations, error {err:.2e}, smallest pivot ratio {worst:.3f}")
    assert st[0] < 200 and err < 1e-7 and worst > 1e-6 and st[7] == 0
    assert np.all(g[:, :, 0].imag == 0) and np.all(g[:, :, 0].real > 0)
    # and the subtraction of every direction with the solved gains leaves nothing; of none, everything
    assert np.abs(R.dd_subtract(g, M, a1, a2, slot=sl, vis=V)).max() < 1e-7 * np.abs(V).max()
    assert np.array_equal(R.dd_subtract(g, M, a1, a2, slot=sl, directions=[], vis=V), V)
    some = R.dd_subtract(g, M, a1, a2, slot=sl, directions=range(1, D), vis=V)
    assert np.abs(some - R.dd_subtract(g, M, a1, a2, slot=sl, directions=[0])).max() < 1e-7 * np.abs(V).max()


def test_subtract_leaves_rows_out_of_range_alone():
    g = np.arange(1, 13).reshape(2, 2, 3) * (1 + 0.5j)
    M = np.arange(1, 9).reshape(2, 4) - 1j
    V = np.array([1 + 1j, 2, 3j, 4])
    a1, a2, sl = [0, 3, 1, 0], [1, 1, -1, 2], [0, 0, 1, 2]
    out = R.dd_subtract(g, M, a1, a2, slot=sl, vis=V)
    assert np.array_equal(out[1:], V[1:])
    assert out[0] == V[0] - g[0, 0, 0] * M[0, 0] * np.conj(g[0, 0, 1]) - g[1, 0, 0] * M[1, 0] * np.conj(g[1, 0, 1])
    assert np.array_equal(R.dd_subtract(g, M, a1, a2, slot=sl)[1:], np.zeros(3))
