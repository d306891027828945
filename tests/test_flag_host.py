"""Residual flagging (gridhip_flag_residuals[_dev], gridhip_imager_flag_dev), the checks that need no GPU: the library, the
header, the ctypes table, both bindings and the hpp carry the three entry points; the header states the semantics; a NULL
context or imager is refused with GRIDHIP_EINVAL whatever else is passed; Context.flag_residuals and Imager.flag hand the
ABI the right pointers, scalar order and NULL for model_vis / group / weights = None (against the recording library of
test_binding_marshalling.py) and refuse wrong dtypes and shapes before any call; flag_groups is right for each `by`; and
the numpy restatement the GPU tests compare with (tests/flag_ref.py) is right on the cases worked by hand
(tests/flag_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flag_ref
from conftest import ROOT
from flag_cases import HAND, hand
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_flag_residuals", "gridhip_flag_residuals_dev", "gridhip_imager_flag_dev"]
f64, c128, i64, u8 = np.float64, np.complex128, np.int64, np.uint8


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
    assert _lib.SIGNATURES["gridhip_flag_residuals"] == _lib.SIGNATURES["gridhip_flag_residuals_dev"]
    assert _lib.load().gridhip_version() >= 240
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 240


def test_header_states_the_semantics():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("residual flagging"):raw.index("int gridhip_flag_residuals(")]
    for phrase in ("FLAGGED ON INPUT", "LEFT ALONE", "NOT FINITE", "ABOVE AMAX", "CLIPPED", "KEPT", "16 + r",  # the classes
                   "LOWER median", "1.4826", "np.sqrt(re * re + im * im)", "hypot",
                   "GRIDHIP_EUNSUPPORTED", "2^18", "262144",                                                  # the limit
                   "G <= 64", "above 64",                                                                     # the LDS boundary
                   "DETERMINISM", "integer atomics only", "no sum of doubles", "same bits"):
        assert phrase in section, phrase
    imager = raw[raw.index("int gridhip_flag_residuals_dev("):raw.index("int gridhip_imager_flag_dev(")]
    assert "DEFINED BY THE CALLS IT REPLACES" in imager and "gridhip_imager_predict_dev" in imager


def test_bindings_carry_the_three():
    import gridhip
    for owner, method in ((gridhip.Context, "flag_residuals"), (gridhip.Imager, "flag"), (gridhip, "flag_groups")):
        assert callable(getattr(owner, method)), method
    assert "flag_groups" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    assert "flagResidualsIO" in head and re.search(r"^flagResidualsIO ::", hs, flags=re.M)
    assert "c_flag_residuals " in hs[hs.index("-- END GENERATED IMPORTS"):]
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bflag_residuals\s*\(", hpp)
    for name in NAMES:
        assert name in hpp, name


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_flag.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    n, G = 4, 2
    grp, vis, mod = np.array([0, 1, 0, 1], dtype=i64), np.full(n, 1 + 2j), np.full(n, 3 + 0j)
    wt, wo, fl, gs, st = np.full(n, 4.0), np.full(n, 8.0), np.full(n, 9, dtype=u8), np.full((G, 4), 5.0), np.full(8, 6.0)
    pg, pv, pm, pw, pwo, pf, pgs, pst = (C.c_void_p(a.ctypes.data) for a in (grp, vis, mod, wt, wo, fl, gs, st))
    cases = [(n, G, pg, 5.0, 0.0, 8, 3), (n, 1, None, 5.0, 1.0, 1, 0), (-1, G, pg, 5.0, 0.0, 8, 3), (n, 0, pg, 5.0, 0.0, 8, 3),
             (n, G, None, 5.0, 0.0, 8, 3), (n, G, pg, 0.0, 0.0, 8, 3), (n, G, pg, float("inf"), 0.0, 8, 3),
             (n, G, pg, 5.0, -1.0, 8, 3), (n, G, pg, 5.0, float("nan"), 8, 3), (n, G, pg, 5.0, 0.0, 0, 3),
             (n, G, pg, 5.0, 0.0, 8, -1), (n, G, pg, 5.0, 0.0, 8, 17), (n, (1 << 18) + 1, pg, 5.0, 0.0, 8, 3)]
    for fn in (lib.gridhip_flag_residuals, lib.gridhip_flag_residuals_dev):
        for (nn, GG, group, nsig, amax, mc, niter) in cases:
            assert fn(None, nn, GG, group, pv, pm, pw, nsig, amax, mc, niter, pwo, pf, pgs, pst) == _lib.EINVAL
            assert fn(None, nn, GG, group, pv, None, None, nsig, amax, mc, niter, pwo, None, None, None) == _lib.EINVAL
        assert fn(None, n, G, pg, None, pm, pw, 5.0, 0.0, 8, 3, None, pf, pgs, pst) == _lib.EINVAL
        assert fn(None, n, G, pg, pv, pm, pw, 5.0, 0.0, 8, 3, pw, pf, pgs, pst) == _lib.EINVAL   # in place
        assert fn(None, n, G, pg, pv, pm, pw, 5.0, 0.0, 8, 3, pv, pf, pgs, pst) == _lib.EINVAL   # wt_out over vis
    for (nn, GG, group, nsig, amax, mc, niter) in cases:
        assert lib.gridhip_imager_flag_dev(None, pwo, pv, GG, group, pw, nsig, amax, mc, niter, pwo, pf, pgs, pst) == _lib.EINVAL
        assert lib.gridhip_imager_flag_dev(None, None, None, GG, group, None, nsig, amax, mc, niter, None, None, None,
                                           None) == _lib.EINVAL
    for a, val in ((vis, 1 + 2j), (mod, 3 + 0j), (wt, 4.0), (wo, 8.0), (fl, 9), (gs, 5.0), (st, 6.0)):
        assert np.all(a == val)


# ---- marshalling: what Context.flag_residuals and Imager.flag hand to the ABI --------------------------------------------
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


N = 6
GROUP = np.array([0, 2, 1, 1, -1, 3], dtype=np.int32)


def awkward_vis():
    vis = (np.arange(2 * N) * (1 - 0.5j)).astype(c128)[::2]  # not contiguous
    mod = (np.arange(N) + 1j).astype(np.complex64)
    assert not vis.flags.c_contiguous
    return vis, mod


def test_flag_residuals_marshalling(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    wt = np.arange(N, dtype=np.float32)
    w, f, g, s = Out(f64, N), Out(u8, N), Out(f64, 3 * 4), Out(f64, 8)
    got = run(lambda: ctx.flag_residuals(vis, mod, group=GROUP, G=3, weights=wt, nsigma=4, amax=2.5, min_count=5, niter=7),
              "gridhip_flag_residuals", N, 3, Arr(GROUP, i64), Arr(vis, c128), Arr(mod, c128), Arr(wt, f64), 4.0, 2.5, 5, 7,
              w, f, g, s)
    assert w.returned(got[0], (N,)) and f.returned(got[1], (N,)) and g.returned(got[2], (3, 4)) and s.returned(got[3], (8,))
    # model_vis, group and weights None are NULL, and G is then 1; the defaults are nsigma 5, amax 0, min_count 8, niter 3;
    # an array already in the ABI's form goes by its own address
    v2 = np.ascontiguousarray(vis)
    got = run(lambda: ctx.flag_residuals(v2), "gridhip_flag_residuals", N, 1, None, Same(v2), None, None, 5.0, 0.0, 8, 3,
              Out(f64, N), Out(u8, N), Out(f64, 4), Out(f64, 8))
    assert got[2].shape == (1, 4) and got[1].dtype == u8
    # in place: out may be the weights themselves, and is what comes back
    w2, g2 = np.ones(N), GROUP.astype(i64)
    got = run(lambda: ctx.flag_residuals(v2, group=g2, G=4, weights=w2, out=w2, niter=0),
              "gridhip_flag_residuals", N, 4, Same(g2), Same(v2), None, Same(w2), 5.0, 0.0, 8, 0, Same(w2), Out(u8, N),
              Out(f64, 16), Out(f64, 8))
    assert got[0] is w2


def test_wrong_dtypes_and_shapes_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    vis, mod = awkward_vis()
    bad = [dict(vis=np.zeros((N, 1), dtype=c128)), dict(model_vis=mod[:-1]), dict(group=GROUP.astype(f64), G=3),
           dict(group=GROUP[:-1], G=3), dict(group=GROUP), dict(G=2), dict(group=GROUP, G=0), dict(weights=np.ones(N - 1)),
           dict(weights=np.ones(N, dtype=c128)), dict(nsigma=0.0), dict(nsigma=-1.0), dict(nsigma=float("inf")),
           dict(nsigma=float("nan")), dict(amax=-1.0), dict(amax=float("nan")), dict(min_count=0), dict(niter=-1),
           dict(niter=17), dict(out=np.zeros(N, dtype=np.float32)), dict(out=np.zeros(N + 1)),
           dict(out=np.zeros(2 * N)[::2])]
    for change in bad:
        with pytest.raises(ValueError):
            ctx.flag_residuals(**{**dict(vis=vis), **change})
    assert rec.calls == []


def test_imager_flag_marshalling(monkeypatch):
    """The scalar order and the NULLs of Imager.flag, with torch CPU tensors standing for device ones (the device back end
    takes an address with data_ptr() whatever the device; only the cuda check is stood in for)."""
    import torch
    import gridhip
    from gridhip import _marshal
    rec = Recorder()
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = rec, None, 0
    monkeypatch.setattr(gridhip.Context, "_use_torch_stream", lambda self: None)
    im = gridhip.Imager(ctx, HANDLE, N, 4, torch.device("cpu"))
    be = _marshal.device()
    monkeypatch.setattr(type(be), "ok", staticmethod(lambda x, dt: x.dtype == dt and x.is_contiguous()))
    try:
        model = torch.zeros((4, 4), dtype=torch.float64)
        vis = torch.arange(N, dtype=torch.float64).to(torch.complex128)
        grp, wt = torch.tensor([0, 1, 0, 1, 5, -1]), torch.ones(N, dtype=torch.float64)

        class At:  # the argument is this tensor's own address
            def __init__(self, t):
                self.t = t

            def check(self, arg, where):
                assert arg.value == self.t.data_ptr(), where
        rec.expect("gridhip_imager_flag_dev", HANDLE, (At(model), At(vis), 2, At(grp), At(wt), 3.0, 9.5, 2, 4, At(wt),
                                                        Out(u8, N), Out(f64, 8), Out(f64, 8)))
        w, f, g, s = im.flag(model, vis, group=grp, G=2, weights=wt, nsigma=3, amax=9.5, min_count=2, niter=4, out=wt)
        assert w is wt and f.dtype == torch.uint8 and tuple(g.shape) == (2, 4) and tuple(s.shape) == (8,)
        assert f.tolist() == [1, 2, 3, 4, 5, 6]
        rec.expect("gridhip_imager_flag_dev", HANDLE, (At(model), At(vis), 1, None, None, 5.0, 0.0, 8, 3, Out(f64, N),
                                                        Out(u8, N), Out(f64, 4), Out(f64, 8)))
        w, f, g, s = im.flag(model, vis)
        assert w.tolist() == [1, 2, 3, 4, 5, 6] and tuple(g.shape) == (1, 4)
        assert rec.calls == ["gridhip_imager_flag_dev"] * 2
        for kw in (dict(group=grp), dict(G=3), dict(group=grp[:-1], G=2), dict(weights=wt[:-1]), dict(niter=17),
                   dict(nsigma=0), dict(out=torch.ones(N, dtype=torch.float32))):
            with pytest.raises(ValueError):
                im.flag(model, vis, **kw)
        with pytest.raises(ValueError):
            im.flag(model, vis[:-1])
        assert rec.calls == ["gridhip_imager_flag_dev"] * 2
    finally:
        im._h = None


# ---- flag_groups ---------------------------------------------------------------------------------------------------------
def test_flag_groups_for_each_by():
    import torch
    import gridhip
    a1 = [0, 1, 0, 2, 1, 0, 2]
    a2 = [1, 0, 2, 0, 2, 1, 1]   # (0,1) (0,1) (0,2) (0,2) (1,2) (0,1) (1,2): unordered pairs
    slot = [0, 0, 0, 1, 1, 1, 1]
    g, G = gridhip.flag_groups(a1, a2)
    assert G == 3 and g.dtype == torch.int64 and g.tolist() == [0, 0, 1, 1, 2, 0, 2]
    g, G = gridhip.flag_groups(a1, a2, slot, by="slot")
    assert G == 2 and g.tolist() == slot
    g, G = gridhip.flag_groups(a1, a2, [5, 5, 5, 9, 9, 9, 9], by="slot")  # compact ids
    assert G == 2 and g.tolist() == slot
    g, G = gridhip.flag_groups(a1, a2, slot, by="baseline_slot")
    # the sorted keys: (0,1,0) (0,1,1) (0,2,0) (0,2,1) (1,2,1)
    assert G == 5 and g.tolist() == [0, 0, 2, 3, 4, 1, 4]
    g, G = gridhip.flag_groups(a1, a2, by="all")
    assert G == 1 and g.tolist() == [0] * 7
    g, G = gridhip.flag_groups(np.array(a1, dtype=np.int32), torch.tensor(a2))
    assert G == 3 and g.tolist() == [0, 0, 1, 1, 2, 0, 2]
    g, G = gridhip.flag_groups([], [])
    assert G == 1 and g.numel() == 0
    for kw in (dict(by="antenna"), dict(by="slot"), dict(by="baseline_slot"), dict(slot=[0, 1], by="slot")):
        with pytest.raises(ValueError):
            gridhip.flag_groups(a1, a2, **kw)
    with pytest.raises(ValueError):
        gridhip.flag_groups(a1, a2[:-1])


# ---- the numpy restatement on the cases worked by hand -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_on_hand_cases(name):
    vis, kw, codes, gstats, stats = hand(name)
    w, f, g, s = flag_ref.flag_residuals(vis, **kw)
    assert np.array_equal(f, codes)
    assert flag_ref.same_bits(g, gstats)
    assert np.array_equal(s, stats)
    assert flag_ref.same_bits(w, np.where(codes == 0, 1.0, 0.0))


def test_restatement_rounds_and_classes():
    vis, kw, codes, _, _ = hand("two_rounds")
    # niter = 1 is the first round alone: the statistics are those round 0 saw
    w, f, g, s = flag_ref.flag_residuals(vis, **{**kw, "niter": 1})
    assert f.tolist() == [0] * 8 + [16] and list(g[0, :3]) == [9, 10.0, 8.0] and list(s[[0, 2, 7]]) == [1, 1, 8]
    # niter = 0: no statistics, the count alone
    w, f, g, s = flag_ref.flag_residuals(vis, **{**kw, "niter": 0})
    assert not f.any() and g[0, 0] == 9 and np.isnan(g[0, 1:3]).all() and g[0, 3] == np.inf and list(s[[0, 1, 7]]) == [0, 9, 9]
    # the classes, the first that applies: a flagged NaN, a left-alone NaN (its weight intact), an unflagged NaN, 1e200
    # (its square overflows), one above amax, and four ordinary ones
    v = np.array([np.nan, np.nan, np.nan, 1e200, 50, 1, 2, 3, 4], dtype=c128)
    wt = np.array([0.0, 2.5, 1, 1, 1, 1, 1, -1.0, np.nan])
    grp = np.array([0, 7, 0, 0, 0, 0, 0, 0, 0])
    w, f, g, s = flag_ref.flag_residuals(v, group=grp, G=1, weights=wt, amax=10.0, min_count=1, niter=2)
    assert f.tolist() == [1, 2, 3, 3, 4, 0, 0, 1, 1]
    assert w.tolist() == [0, 2.5, 0, 0, 0, 1, 1, 0, 0] and not np.signbit(w).any()
    assert s.tolist() == [1, 2, 0, 2, 1, 1, 3, 2] and list(g[0, :3]) == [2, 1.0, 0.0]
    # a model: the residual is what is tested; the amplitude is sqrt(re * re + im * im), not hypot
    w, f, g, s = flag_ref.flag_residuals(np.array([3 + 4j] * 3), np.array([0j, 3 + 4j, 6 + 8j]), min_count=1, niter=1)
    assert list(g[0]) == [3, 5.0, 0.0, np.inf]
    x = np.array([1e-200 + 1e-200j])
    assert flag_ref.amplitude(x)[0] == 0.0 and np.abs(x)[0] > 0.0
