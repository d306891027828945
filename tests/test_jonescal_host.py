"""Polarisation (gridhip_jonescal*, gridhip_apply_jones*, gridhip_stokes*), the checks that need no GPU: the library, the
header, the ctypes table, both bindings and the hpp carry the six entry points; a NULL context is refused with
GRIDHIP_EINVAL whatever else is passed; Context.jonescal, apply_jones and stokes hand the ABI the right pointers, scalar
order and NULLs (against the recording library of test_binding_marshalling.py) and refuse wrong dtypes and shapes before
any call; and the numpy restatement the GPU tests compare with (tests/jonescal_ref.py) is right on cases small enough to
verify by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gaincal_ref
import jonescal_ref as J
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_jonescal", "gridhip_jonescal_dev", "gridhip_apply_jones", "gridhip_apply_jones_dev", "gridhip_stokes",
         "gridhip_stokes_dev"]
f64, c128, i64 = np.float64, np.complex128, np.int64


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_six():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    for name in NAMES[::2]:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name + "_dev"]
    assert re.search(r"\bint64_t gridhip_jonescal_lds_antennas\s*\(void\)", src)
    assert _lib.load().gridhip_version() >= 280
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 280
    # the section stands after direction-dependent calibration and states the semantics
    assert raw.index("direction-dependent calibration:") < raw.index("---- polarisation:") < raw.index("int gridhip_jonescal(")
    block = raw[raw.index("---- polarisation:"):raw.index("int gridhip_stokes(")]
    for phrase in ("GRIDHIP_EUNSUPPORTED", "2^21", "DETERMINISM", "LDS BUDGET", "FLAGGED", "DROPPED", "AUTO", "UNSOLVED",
                   "1e-12", "LDL^H", "no fused multiply-add", "scalar approximation", "gauge"):
        assert phrase in block, phrase


def test_bindings_carry_the_six():
    import gridhip
    for method in ("jonescal", "apply_jones", "stokes"):
        assert callable(getattr(gridhip.Context, method)), method
    assert "jonescal_lds_antennas" in gridhip.__all__
    lim = gridhip.jonescal_lds_antennas()
    assert isinstance(lim, int) and lim >= 64 and lim * 160 <= 160 * 1024  # 160 B per antenna, within a CU's LDS
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES + ["gridhip_jonescal_lds_antennas"]:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("jonescalIO", "applyJonesIO", "stokesIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bjonescal\s*\(", hpp) and re.search(r"\bapply_jones\s*\(", hpp) and re.search(r"\bstokes\s*\(", hpp)
    for name in NAMES:
        assert name in hpp, name


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_jonescal.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    n, A, T = 3, 3, 1
    a1, a2, sl = np.array([0, 0, 1], dtype=i64), np.array([1, 2, 2], dtype=i64), np.zeros(n, dtype=i64)
    vis, mod, out = np.full((n, 2, 2), 1 + 2j), np.full((n, 2, 2), 3 + 0j), np.full((n, 2, 2), 7 + 7j)
    wt, wo, g, st, sk = np.full(n, 4.0), np.full(n, 8.0), np.full((T, A, 2, 2), 5 + 5j), np.full(8, 6.0), np.full((4, n), 9 - 9j)
    p1, p2, ps, pv, pm, po, pw, pwo, pg, pst, psk = (C.c_void_p(a.ctypes.data)
                                                     for a in (a1, a2, sl, vis, mod, out, wt, wo, g, st, sk))
    for fn in (lib.gridhip_jonescal, lib.gridhip_jonescal_dev):
        for (nn, AA, TT, slot, mode, ref, niter, tol) in [
                (n, A, T, ps, 0, 0, 5, 1e-8), (n, A, T, None, 2, -1, 0, 0.0), (-1, A, T, ps, 0, 0, 5, 0.0),
                (n, 1, T, ps, 0, 0, 5, 0.0), (n, A, 0, ps, 0, 0, 5, 0.0), (n, A, 2, None, 0, 0, 5, 0.0),
                (n, A, T, ps, 3, 0, 5, 0.0), (n, A, T, ps, 0, A, 5, 0.0), (n, A, T, ps, 0, 0, -1, 0.0),
                (n, A, T, ps, 0, 0, 5, -1.0), (n, A, T, ps, 0, 0, 5, float("nan")), (n, 1 << 11, 1 << 11, ps, 0, 0, 1, 0.0)]:
            assert fn(None, nn, AA, TT, p1, p2, slot, pv, pm, pw, mode, ref, 0, niter, tol, pg, pst) == _lib.EINVAL
            assert fn(None, nn, AA, TT, p1, p2, slot, pv, pm, None, mode, ref, 1, niter, tol, pg, None) == _lib.EINVAL
        assert fn(None, n, A, T, p1, p2, ps, pv, pm, pw, 0, 0, 0, 5, 0.0, pv, pst) == _lib.EINVAL  # gains over vis
    for fn in (lib.gridhip_apply_jones, lib.gridhip_apply_jones_dev):
        for inverse in (1, 0, 2, -1):
            assert fn(None, n, A, T, p1, p2, ps, pg, inverse, pv, pw, po, pwo) == _lib.EINVAL
            assert fn(None, n, A, T, p1, p2, None, pg, inverse, pv, None, pv, None) == _lib.EINVAL  # in place
    for fn in (lib.gridhip_stokes, lib.gridhip_stokes_dev):
        for basis, which, inverse in ((0, 15, 0), (1, 1, 0), (0, 15, 1), (2, 15, 0), (0, 0, 0), (0, 16, 0), (0, 7, 1)):
            assert fn(None, n, basis, which, inverse, pv, psk) == _lib.EINVAL
    for a, val in ((vis, 1 + 2j), (mod, 3 + 0j), (out, 7 + 7j), (wt, 4.0), (wo, 8.0), (g, 5 + 5j), (st, 6.0), (sk, 9 - 9j)):
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


def awkward_vis():
    vis = (np.arange(2 * N * 4).reshape(2 * N, 2, 2) * (1 - 0.5j)).astype(c128)[::2]  # not contiguous
    mod = (np.arange(N * 4).reshape(N, 2, 2) + 1j).astype(np.complex64)
    assert not vis.flags.c_contiguous
    return vis, mod


def test_jonescal_marshalling(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    wt = np.arange(N, dtype=np.float32)
    for mode, code in (("full", 0), ("diagonal", 1), ("phase", 2)):
        g_out, st_out = Out(c128, 2 * 3 * 4), Out(f64, 8)
        g, st = run(lambda: ctx.jonescal(vis, mod, A1, A2, 3, slot=SLOT, nslots=2, weights=wt, mode=mode, refant=None,
                                         niter=7, tol=1e-6),
                    "gridhip_jonescal", N, 3, 2, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(vis, c128), Arr(mod, c128),
                    Arr(wt, f64), code, -1, 0, 7, 1e-6, g_out, st_out)
        assert g_out.returned(g, (2, 3, 2, 2)) and st_out.returned(st, (8,))
    # slot=None and weights=None are NULL; arrays already in the ABI's form go by their own address; a given gains is the
    # warm start, updated in place and returned
    v2, m2 = np.ascontiguousarray(vis), np.ascontiguousarray(mod, dtype=c128)
    a1, a2 = np.array(A1, dtype=i64), np.array(A2, dtype=i64)
    warm = np.ones((1, 3, 2, 2), dtype=c128)
    g, st = run(lambda: ctx.jonescal(v2, m2, a1, a2, 3, gains=warm),
                "gridhip_jonescal", N, 3, 1, Same(a1), Same(a2), None, Same(v2), Same(m2), None, 0, 0, 1, 50, 1e-8,
                Same(warm), Out(f64, 8))
    assert g is warm


def test_apply_jones_marshalling(rig):
    ctx, rec, run = rig
    vis, _ = awkward_vis()
    gains = (np.arange(24).reshape(2, 3, 2, 2) + 2j).astype(np.complex64)
    wt = np.arange(N, dtype=f64)
    o, w = Out(c128, 4 * N), Out(f64, N)
    vo, wo = run(lambda: ctx.apply_jones(gains, vis, A1, A2, slot=SLOT, weights=wt),
                 "gridhip_apply_jones", N, 3, 2, Arr(A1, i64), Arr(A2, i64), Arr(SLOT, i64), Arr(gains, c128), 1,
                 Arr(vis, c128), Same(wt), o, w)
    assert o.returned(vo, (N, 2, 2)) and w.returned(wo, (N,))
    # one interval, no weights, corrupting a model, in place
    g1, v2 = np.ones((1, 3, 2, 2), dtype=c128), np.ascontiguousarray(vis)
    wout = np.zeros(N)
    vo, wo = run(lambda: ctx.apply_jones(g1, v2, A1, A2, inverse=False, out=v2, weights_out=wout),
                 "gridhip_apply_jones", N, 3, 1, Arr(A1, i64), Arr(A2, i64), None, Same(g1), 0, Same(v2), None, Same(v2),
                 Same(wout))
    assert vo is v2 and wo is wout


def test_stokes_marshalling(rig):
    ctx, rec, run = rig
    vis, _ = awkward_vis()
    o = Out(c128, 4 * N)
    s = run(lambda: ctx.stokes(vis), "gridhip_stokes", N, 0, 15, 0, Arr(vis, c128), o)
    assert o.returned(s, (4, N))
    v2, block = np.ascontiguousarray(vis), np.zeros((4, N), dtype=c128)
    for which, mask in (("I", 1), ("q", 2), ("UV", 12), ("VI", 9), ("IQUV", 15)):
        s = run(lambda: ctx.stokes(v2, basis="circular", which=which, out=block),
                "gridhip_stokes", N, 1, mask, 0, Same(v2), Same(block))
        assert s is block
    # the inverse: the (4, n) block is the input and goes fifth as the output does in the forward form - vis is written
    o = Out(c128, 4 * N)
    blk32 = np.arange(4 * N).reshape(4, N).astype(np.complex64)
    v = run(lambda: ctx.stokes(blk32, inverse=True), "gridhip_stokes", N, 0, 15, 1, o, Arr(blk32, c128))
    assert o.returned(v, (N, 2, 2))
    out = np.zeros((N, 2, 2), dtype=c128)
    v = run(lambda: ctx.stokes(block, basis="circular", inverse=True, out=out),
            "gridhip_stokes", N, 1, 15, 1, Same(out), Same(block))
    assert v is out


def test_wrong_dtypes_and_shapes_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    ok = dict(vis=vis, model_vis=mod, a1=A1, a2=A2, nant=3)
    bad = [dict(a1=np.array(A1, dtype=f64)), dict(a2=A2[:-1]), dict(model_vis=mod[:-1]), dict(vis=np.zeros(N, dtype=c128)),
           dict(vis=np.zeros((N, 4), dtype=c128)), dict(model_vis=np.zeros((N, 2, 3), dtype=c128)), dict(model_vis=None),
           dict(slot=SLOT.astype(np.float32), nslots=2), dict(slot=SLOT[:-1], nslots=2), dict(nslots=2), dict(nant=1),
           dict(nslots=0, slot=SLOT), dict(weights=np.ones(N - 1)), dict(weights=np.ones(N, dtype=c128)),
           dict(weights=np.ones((N, 4))), dict(gains=np.ones((1, 3, 2, 2), dtype=np.complex64)),
           dict(gains=np.ones((1, 3), dtype=c128)), dict(gains=np.ones((3, 1, 2, 2), dtype=c128)),
           dict(gains=np.ones((1, 6, 2, 2), dtype=c128)[:, ::2]), dict(refant=3), dict(niter=-1), dict(tol=-1.0),
           dict(tol=float("nan")), dict(mode="amplitude"), dict(mode=0), dict(mode=True)]
    for change in bad:
        with pytest.raises(ValueError):
            ctx.jonescal(**{**ok, **change})
    g = np.ones((2, 3, 2, 2), dtype=c128)
    for kw in [dict(gains=np.ones((2, 3), dtype=c128)), dict(gains=np.ones((2, 3, 2, 1), dtype=c128)),
               dict(a1=np.array(A1, dtype=f64)), dict(slot=None), dict(vis=np.zeros(N, dtype=c128)),
               dict(out=np.zeros((N, 2, 2), dtype=np.complex64)), dict(out=np.zeros((N + 1, 2, 2), dtype=c128)),
               dict(out=np.zeros(4 * N, dtype=c128)), dict(weights_out=np.zeros(N, dtype=np.float32)),
               dict(weights=np.ones(N + 1))]:
        args = {**dict(gains=g, vis=vis, a1=A1, a2=A2, slot=SLOT), **kw}
        with pytest.raises(ValueError):
            ctx.apply_jones(args.pop("gains"), args.pop("vis"), args.pop("a1"), args.pop("a2"), **args)
    blk = np.zeros((4, N), dtype=c128)
    for kw in [dict(vis=np.zeros(N, dtype=c128)), dict(vis=np.zeros((N, 4), dtype=c128)), dict(basis="xy"), dict(basis=0),
               dict(which=""), dict(which="IX"), dict(which="II"), dict(which=15), dict(out=np.zeros((N, 4), dtype=c128)),
               dict(out=np.zeros((4, N), dtype=np.complex64)), dict(out=np.zeros((4, 2 * N), dtype=c128)[:, ::2]),
               dict(vis=blk, inverse=True, which="IQU"), dict(vis=np.zeros((3, N), dtype=c128), inverse=True),
               dict(vis=vis, inverse=True), dict(vis=blk, inverse=True, out=np.zeros((4, N), dtype=c128)),
               dict(vis=blk, inverse=True, out=np.zeros((N, 2, 2), dtype=np.complex64))]:
        with pytest.raises(ValueError):
            ctx.stokes(**{**dict(vis=vis), **kw})
    assert rec.calls == []


# ---- the numpy restatement on cases small enough to verify by hand -------------------------------------------------------
def mat(x):
    return np.array(x, dtype=c128).reshape(2, 2)


def test_one_visibility_two_antennas_from_the_identity():
    """G = I: toward p, Z = M, num = s V M^H, den = s M M^H; toward q, Z = M^H, num = s V^H M, den = s M^H M.  Against numpy's
    own matrix algebra (another rounding order: 1e-14)."""
    V, M, s = mat([2 + 1j, 0.5 - 1j, -1 + 0.25j, 1 + 3j]), mat([1 + 1j, 0.5j, 0.25 - 0.5j, 2 - 1j]), 0.75
    for a1, a2 in (([0], [1]), ([1], [0])):
        G, st = J.jonescal(V[None], M[None], a1, a2, 2, wt=[s], refant=-1, niter=1, tol=0)
        p, q = a1[0], a2[0]
        want_p = (s * V @ M.conj().T) @ np.linalg.inv(s * M @ M.conj().T)
        want_q = (s * V.conj().T @ M) @ np.linalg.inv(s * M.conj().T @ M)
        assert np.allclose(G[0, p], want_p, rtol=1e-13, atol=1e-14) and np.allclose(G[0, q], want_q, rtol=1e-13, atol=1e-14)
        assert list(st[[0, 4, 5, 6, 7]]) == [1, 1, 0, 0, 0]  # one visibility makes both antennas solvable
        assert st[3] == pytest.approx(s * (np.abs(V - M) ** 2).sum(), rel=1e-14)
        want = np.stack([want_p, want_q] if p == 0 else [want_q, want_p])
        assert st[1] == pytest.approx(np.sqrt((np.abs(want - np.eye(2)) ** 2).sum() / (np.abs(want) ** 2).sum()), rel=1e-12)
        r = V - G[0, p] @ M @ G[0, q].conj().T
        assert st[2] == pytest.approx(s * (np.abs(r) ** 2).sum(), rel=1e-12)
        # the diagonal modes use the same sums with only their diagonals
        Gd, std = J.jonescal(V[None], M[None], a1, a2, 2, wt=[s], refant=-1, niter=1, tol=0, mode=1)
        num, den = s * V @ M.conj().T, s * M @ M.conj().T
        assert Gd[0, p, 0, 0] == pytest.approx(num[0, 0] / den[0, 0].real, rel=1e-14)
        assert Gd[0, p, 1, 1] == pytest.approx(num[1, 1] / den[1, 1].real, rel=1e-14)
        assert np.all(Gd[..., 0, 1] == 0) and np.all(Gd[..., 1, 0] == 0) and not np.signbit(Gd[..., 0, 1].real).any()
        Gp, _ = J.jonescal(V[None], M[None], a1, a2, 2, wt=[s], refant=-1, niter=1, tol=0, mode=2)
        assert np.allclose(np.abs(Gp[0, :, [0, 1], [0, 1]]), 1, rtol=1e-15, atol=0)
        assert np.allclose(np.angle(Gp[0, :, [0, 1], [0, 1]]), np.angle(Gd[0, :, [0, 1], [0, 1]]), rtol=1e-14, atol=0)


def test_the_rotation_takes_out_one_common_phase():
    rng = np.random.default_rng(3)
    a1, a2, sl, V, M, _ = polarised(rng, 4, 2)
    G0, s0 = J.jonescal(V, M, a1, a2, 4, slot=sl, T=2, refant=-1, niter=5, tol=0)
    G1, s1 = J.jonescal(V, M, a1, a2, 4, slot=sl, T=2, refant=2, niter=5, tol=0)
    for t in (0, 1):
        r = G0[t, 2, 0, 0]
        assert np.allclose(G1[t], G0[t] * (np.conj(r) / abs(r)), rtol=1e-14, atol=1e-15)
        assert G1[t, 2, 0, 0].imag == 0 and G1[t, 2, 0, 0].real == pytest.approx(abs(r), rel=1e-15)
    assert s1[2] == pytest.approx(s0[2], rel=1e-10)  # chi^2 does not see a common phase


def polarised(rng, A, T, diagonal=False, noise=0.0):
    """every baseline of A antennas in T intervals, a strongly polarised model (the gauge is then fixed up to a phase and
    the solve converges quickly), Jones matrices I + 0.2 (N + iN) -> a1, a2, slot, V, M, the true Jones matrices"""
    p, q = np.triu_indices(A, 1)
    a1, a2, sl = np.tile(p, T), np.tile(q, T), np.repeat(np.arange(T), len(p))
    n = len(a1)
    Gt = np.zeros((T, A, 2, 2), dtype=c128)
    Gt[..., 0, 0] = Gt[..., 1, 1] = 1
    Gt += 0.2 * (rng.normal(size=Gt.shape) + 1j * rng.normal(size=Gt.shape))
    if diagonal:
        Gt[..., 0, 1] = Gt[..., 1, 0] = 0
    M = rng.normal(size=(n, 2, 2)) + 1j * rng.normal(size=(n, 2, 2))
    V = J.mm(J.mm(Gt[sl, a1], M), J.herm(Gt[sl, a2]))
    V = V + noise * (rng.normal(size=V.shape) + 1j * rng.normal(size=V.shape))
    return a1, a2, sl, V, M, Gt


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_gains_and_a_scalar_model_reproduce_gaincal(mode):
    """G = g I and M = m I: every 2x2 sum is the scalar one on its diagonal (twice over in rel, chi^2: the factor cancels in
    rel and is 2 in chi^2), so all three modes reproduce gaincal_ref.gaincal on the scalar stream - mode 2 its phase-only
    mode."""
    rng = np.random.default_rng(20 + mode)
    a1, a2, sl, V, M, _ = polarised(rng, 5, 2)
    v, m, w = V[:, 0, 0], M[:, 0, 0] + 2, rng.uniform(0.5, 2, len(a1))
    z = np.zeros_like(v)
    Vs, Ms = np.stack([v, z, z, v], 1).reshape(-1, 2, 2), np.stack([m, z, z, m], 1).reshape(-1, 2, 2)
    for niter in (1, 2, 7):
        G, st = J.jonescal(Vs, Ms, a1, a2, 5, slot=sl, T=2, wt=w, niter=niter, tol=0, mode=mode, refant=1)
        g, sg = gaincal_ref.gaincal(v, m, a1, a2, 5, slot=sl, T=2, wt=w, niter=niter, tol=0, mode=int(mode == 2), refant=1)
        scale = np.abs(g).max()
        assert np.abs(G[..., 0, 0] - g).max() <= 1e-14 * scale and np.abs(G[..., 1, 1] - g).max() <= 1e-14 * scale
        assert np.all(G[..., 0, 1] == 0) and np.all(G[..., 1, 0] == 0)
        assert np.array_equal(st[[0, 4, 5, 6, 7]], sg[[0, 4, 5, 6, 7]])
        assert st[1] == pytest.approx(sg[1], rel=1e-12) and st[2] == pytest.approx(2 * sg[2], rel=1e-10)
        assert st[3] == pytest.approx(2 * sg[3], rel=1e-14)


def test_noise_free_data_are_recovered_and_an_unpolarised_model_is_not_solvable():
    rng = np.random.default_rng(4)
    a1, a2, sl, V, M, Gt = polarised(rng, 7, 3)
    G, st = J.jonescal(V, M, a1, a2, 7, slot=sl, T=3, niter=300, tol=1e-13)
    assert st[0] < 300 and st[2] <= 1e-14 * st[3] and st[7] == 0
    assert np.abs(J.mm(J.mm(G[sl, a1], M), J.herm(G[sl, a2])) - V).max() <= 1e-10 * np.abs(V).max()
    a1, a2, sl, V, M, Gt = polarised(rng, 7, 3, diagonal=True)
    G, st = J.jonescal(V, M, a1, a2, 7, slot=sl, T=3, niter=300, tol=1e-13, mode=1)
    assert st[0] < 300 and st[2] <= 1e-14 * st[3] and np.all(G[..., 0, 1] == 0)
    # only XX non-zero: den is singular for every antenna - all unsolved in both modes, every gain the identity
    M1 = np.zeros_like(M)
    M1[:, 0, 0] = M[:, 0, 0]
    for mode in (0, 1):
        G, st = J.jonescal(V, M1, a1, a2, 7, slot=sl, T=3, niter=4, tol=0, mode=mode)
        assert st[7] == 21 and st[1] == 0 and np.array_equal(G, np.broadcast_to(np.eye(2), G.shape))


def test_flagged_samples_are_selected_out():
    rng = np.random.default_rng(5)
    a1, a2, sl, V, M, _ = polarised(rng, 4, 1, noise=0.05)
    G0, s0 = J.jonescal(V, M, a1, a2, 4, niter=4, tol=0)
    Vx, Mx = np.concatenate([V, np.full((3, 2, 2), np.nan)]), np.concatenate([M, np.full((3, 2, 2), np.inf)])
    G1, s1 = J.jonescal(Vx, Mx, np.append(a1, [0, 1, 2]), np.append(a2, [1, 2, 3]), 4,
                        wt=np.append(np.ones(len(a1)), [0, -1, np.nan]), niter=4, tol=0)
    assert np.array_equal(G1, G0) and s1[5] == 3 and np.array_equal(s1[[0, 1, 2, 3, 4, 6, 7]], s0[[0, 1, 2, 3, 4, 6, 7]])


def test_stokes_forward_of_inverse_is_the_identity_to_the_bit():
    """values with short mantissas: every sum and difference is exact, so the round trip gives the very bits, in both bases"""
    rng = np.random.default_rng(6)
    S = (rng.integers(-64, 64, (4, 50)) + 1j * rng.integers(-64, 64, (4, 50))) / 8
    for basis in (0, 1):
        V = J.stokes_inverse(S, basis)
        assert J.stokes(V, basis).tobytes() == S.astype(c128).tobytes()
        back = J.stokes_inverse(J.stokes(V, basis), basis)
        assert back.tobytes() == V.tobytes()
    # the definitions themselves, on one sample
    V = mat([3 + 1j, 0.5 - 2j, 1.5 + 4j, 1 - 3j])[None]
    a, b, c, d = V[0].ravel()
    assert np.array_equal(J.stokes(V, 0)[:, 0], [(a + d) / 2, (a - d) / 2, (b + c) / 2, (b - c) / 2j])
    assert np.array_equal(J.stokes(V, 1)[:, 0], [(a + d) / 2, (b + c) / 2, (b - c) / 2j, (a - d) / 2])
    part = J.stokes(V, 0, which=0b0101, out=np.full((4, 1), 7 + 7j))
    assert np.array_equal(part[:, 0], [(a + d) / 2, 7 + 7j, (b + c) / 2, 7 + 7j])


def test_apply_inverse_after_forward_returns_the_input():
    rng = np.random.default_rng(7)
    a1, a2, sl, V, M, Gt = polarised(rng, 5, 2)
    w = rng.uniform(0.5, 2, len(a1))
    Vc, wc = J.apply_jones(Gt, M, a1, a2, slot=sl, wt=w, inverse_=False)
    assert np.array_equal(wc, w) and np.abs(Vc - V).max() == 0  # (polarised() corrupts in the very same way)
    Vb, wb = J.apply_jones(Gt, Vc, a1, a2, slot=sl, wt=w)
    assert np.abs(Vb - M).max() <= 1e-13 * np.abs(M).max()
    det = np.abs(np.linalg.det(Gt))
    assert np.allclose(wb, w * det[sl, a1] * det[sl, a2], rtol=1e-14, atol=0)
    # G = g I is apply_gains on each correlation, weights included
    g = (1 + 0.3 * rng.normal(size=(2, 5))) * np.exp(1j * rng.uniform(-2, 2, (2, 5)))
    Gs = g[..., None, None] * np.eye(2)
    Vj, wj = J.apply_jones(Gs, V, a1, a2, slot=sl, wt=w)
    for i in (0, 1):
        for j in (0, 1):
            vs, ws = gaincal_ref.apply_gains(g, V[:, i, j], a1, a2, slot=sl, wt=w)
            assert np.abs(Vj[:, i, j] - vs).max() <= 1e-14 * np.abs(vs).max() and np.allclose(wj, ws, rtol=1e-14, atol=0)
    # a singular matrix, an index out of range: the sample is kept and its weight is +0.0
    Gb = Gt.copy()
    Gb[0, 1] = [[1, 2], [2, 4]]
    Vo, wo = J.apply_jones(Gb, V, np.where(np.arange(len(a1)) == 5, -1, a1), a2, slot=sl, wt=w)
    hit = ((sl == 0) & ((a1 == 1) | (a2 == 1))) | (np.arange(len(a1)) == 5)
    assert np.array_equal(Vo[hit], V[hit]) and np.all(wo[hit] == 0) and np.all(wo[~hit] > 0)
