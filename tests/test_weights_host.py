"""Imaging weights (gridhip_weights*, gridhip_imager_create*_weighted_dev, gridhip_imager_weight_stats_dev), the checks that
need no GPU: the library, the header, the ctypes table, both bindings and the hpp carry the five entry points; a NULL
context or imager is refused with GRIDHIP_EINVAL whatever else is passed; Context.weights, Context.imager(weighting=...)
and Imager.weight_stats hand the ABI the right pointers, scalar order and NULL for weights=None (against the recording
library of test_binding_marshalling.py) and refuse wrong dtypes, shapes and mode names before any call; and the numpy
restatement the GPU tests compare with (tests/weights_ref.py) is right on cases computed by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import weights_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Ref, Same, address

NAMES = ["gridhip_weights", "gridhip_weights_dev", "gridhip_imager_create_weighted_dev",
         "gridhip_imager_create_aw_weighted_dev", "gridhip_imager_weight_stats_dev"]
f64, c128, i64 = np.float64, np.complex128, np.int64
THETA, LAM, NPIX = 0.008, 2000, 16  # gridhip_image_size(0.008, 2000) = 16


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_weights():
    from gridhip import _lib
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_weights"] == _lib.SIGNATURES["gridhip_weights_dev"]
    # the weighted creations are the plain ones plus (mode, robust, taper_sigma, wt_in) before the handle's address
    extra = [C.c_int, C.c_double, C.c_double, C.c_void_p]
    for plain, weighted in (("gridhip_imager_create_dev", "gridhip_imager_create_weighted_dev"),
                            ("gridhip_imager_create_aw_dev", "gridhip_imager_create_aw_weighted_dev")):
        a, b = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[weighted][1]
        assert b == a[:-1] + extra + a[-1:], weighted
    assert _lib.load().gridhip_version() >= 180
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 180


def test_bindings_carry_the_weights():
    import gridhip
    for owner, method in ((gridhip.Context, "weights"), (gridhip.Imager, "weight_stats")):
        assert callable(getattr(owner, method)), method
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("weightsIO", "imagerCreateWeightedIO", "imagerCreateAwWeightedIO", "imagerWeightStatsIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert re.search(r"\bweights\s*\(", hpp) and "gridhip_weights" in hpp


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_weights.py::test_refusals); here: a NULL handle is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    n = 5
    u, v, s, w, st = np.full(n, 1.0), np.full(n, 2.0), np.full(n, 3.0), np.full(n, 4.0), np.full(8, 5.0)
    pu, pv, ps, pw, pst = (C.c_void_p(a.ctypes.data) for a in (u, v, s, w, st))
    h = C.c_void_p()
    for fn in (lib.gridhip_weights, lib.gridhip_weights_dev):
        for mode, robust, sigma in [(1, 0.0, 0.0), (2, 0.5, 10.0), (3, 0.0, 0.0), (-1, 0.0, 0.0), (2, float("nan"), 0.0),
                                    (2, float("inf"), 0.0), (1, 0.0, -1.0), (1, 0.0, float("nan"))]:
            assert fn(None, THETA, LAM, n, pu, pv, 1, ps, mode, robust, sigma, pw, pst) == _lib.EINVAL
            assert fn(None, THETA, LAM, n, pu, pv, 1, None, mode, robust, sigma, pw, None) == _lib.EINVAL
        assert fn(None, THETA, LAM, -1, pu, pv, 1, ps, 1, 0.0, 0.0, pw, pst) == _lib.EINVAL
        assert fn(None, 0.0, LAM, n, pu, pv, 1, ps, 1, 0.0, 0.0, pw, pst) == _lib.EINVAL
        assert fn(None, THETA, LAM, n, None, pv, 1, ps, 1, 0.0, 0.0, None, pst) == _lib.EINVAL
        assert fn(None, THETA, LAM, n, pu, pv, 1, ps, 1, 0.0, 0.0, pu, pst) == _lib.EINVAL  # wt_out overlapping u
        assert fn(None, THETA, LAM, n, pu, pv, 1, pw, 1, 0.0, 0.0, pw, pst) == _lib.EINVAL  # in place
    for mode in (1, 0, 2, 7):
        h.value = 0xDEAD
        assert lib.gridhip_imager_create_weighted_dev(None, 0, 0, 0, 0, 0, 0, None, THETA, LAM, n, pu, pv, None, 1, mode, 0.0,
                                                      0.0, ps, C.byref(h)) == _lib.EINVAL
        assert not h.value  # (a refused creation leaves NULL)
        h.value = 0xDEAD
        assert lib.gridhip_imager_create_aw_weighted_dev(None, THETA, LAM, 1, 1, 1, 1, pu, pu, pu, n, pu, pv, pu, 1, None,
                                                         None, mode, 0.0, 0.0, None, C.byref(h)) == _lib.EINVAL
        assert not h.value
    assert lib.gridhip_imager_weight_stats_dev(None, pst) == _lib.EINVAL
    assert lib.gridhip_imager_weight_stats_dev(None, None) == _lib.EINVAL
    for a, val in ((u, 1.0), (v, 2.0), (s, 3.0), (w, 4.0), (st, 5.0)):
        assert np.all(a == val)


# ---- the numpy restatement on cases computed by hand ---------------------------------------------------------------------
def three_in_two_cells():
    """N = 4, lam = 4: p = u / 4 and the cell is x = 2 + floor(4 p + 0.5) = 2 + round(u).  Visibilities 0 and 1 share cell
    (y, x) = (2, 3), visibility 2 sits alone in (1, 2)."""
    u = np.array([1.0, 1.2, 0.0])
    v = np.array([0.0, -0.2, -1.0])
    return 4, 4, u, v


def test_three_visibilities_in_two_cells():
    N, lam, u, v = three_in_two_cells()
    assert list(weights_ref.cells(N, lam, u, v)) == [2 * 4 + 3, 2 * 4 + 3, 1 * 4 + 2]
    w, st, D = weights_ref.weights(N, lam, u, v, "natural")
    assert list(w) == [1.0, 1.0, 1.0] and list(st) == [3.0, 3.0, 3.0, 1.0, 0.0, 3.0, 0.0, 0.0]
    w, st, D = weights_ref.weights(N, lam, u, v, "uniform")
    assert list(w) == [0.5, 0.5, 1.0] and D[11] == 2 and D[6] == 1 and D.sum() == 3
    # sum w = 2, sum w^2 / s = 1.5, sum s = 3: noise = sqrt(4.5) / 2
    assert list(st[:3]) == [2.0, 1.5, 3.0] and st[3] == math.sqrt(4.5) / 2 and st[4] == 0.0
    # Briggs, R = 0: sum D^2 / sum D = 5 / 3, f^2 = 25 / (5 / 3) = 15; w = 1 / 31, 1 / 31, 1 / 16
    w, st, D = weights_ref.weights(N, lam, u, v, "briggs", robust=0.0)
    assert st[4] == 25.0 / (5.0 / 3.0) and abs(st[4] - 15.0) < 1e-14
    assert np.allclose(w, [1 / 31, 1 / 31, 1 / 16], rtol=1e-15, atol=0)
    # data weights: s = (2, 4, 3): D = 6 and 3; uniform w = 1/3, 2/3, 1; Briggs: sum D^2 / sum D = 45 / 9 = 5, f^2 = 5
    s = np.array([2.0, 4.0, 3.0])
    w, st, D = weights_ref.weights(N, lam, u, v, "uniform", s=s)
    assert np.allclose(w, [2 / 6, 4 / 6, 1.0], rtol=1e-15, atol=0) and D[11] == 6.0 and D[6] == 3.0
    w, st, D = weights_ref.weights(N, lam, u, v, "briggs", s=s)
    assert st[4] == 5.0 and np.allclose(w, [2 / 31, 4 / 31, 3 / 16], rtol=1e-15, atol=0)
    # a taper of sigma = 1: t = exp(-(u^2 + v^2) / 2)
    w, st, D = weights_ref.weights(N, lam, u, v, "natural", sigma=1.0)
    assert np.allclose(w, np.exp(-np.array([1.0, 1.48, 1.0]) / 2), rtol=1e-15, atol=0)


def scattered(n=4000, N=32, lam=320, seed=5):
    rng = np.random.default_rng(seed)
    u, v = rng.normal(0, 0.2 * lam, n), rng.normal(0, 0.2 * lam, n)
    return N, lam, u, v, rng.uniform(0.5, 2.0, n)


@pytest.mark.parametrize("data_weights", [False, True])
def test_robust_limits(data_weights):
    """R = +8: D f^2 is ~1e-14 D, so w = s (natural) to 1e-12; R = -8: 1 + D f^2 is D f^2 to 1e-15, so w = s / D (uniform)
    up to the one common factor 1 / f^2"""
    N, lam, u, v, s = scattered()
    s = s if data_weights else None
    nat, _, _ = weights_ref.weights(N, lam, u, v, "natural", s=s)
    uni, _, _ = weights_ref.weights(N, lam, u, v, "uniform", s=s)
    hi, _, _ = weights_ref.weights(N, lam, u, v, "briggs", robust=8.0, s=s)
    lo, st, _ = weights_ref.weights(N, lam, u, v, "briggs", robust=-8.0, s=s)
    inside = weights_ref.cells(N, lam, u, v) >= 0
    assert inside.sum() > 3000
    assert np.abs(hi / nat - 1).max() < 1e-12
    ratio = (lo / uni)[inside]
    assert np.abs(ratio / ratio[0] - 1).max() < 1e-12 and abs(ratio[0] * st[4] - 1) < 1e-12
    assert np.array_equal(lo[~inside], nat[~inside])  # outside the grid every mode keeps s t


def test_flagged_and_outside_bookkeeping():
    N, lam, u, v = three_in_two_cells()
    u = np.concatenate([u, [1.0, 100.0, np.nan, 1.0, 1.0]])
    v = np.concatenate([v, [0.0, 0.0, 0.0, 0.0, 0.0]])
    s = np.array([2.0, 4.0, 3.0, 0.0, 5.0, 6.0, -1.0, np.nan])  # 3: zero, 6: negative, 7: NaN are flagged; 4, 5 outside
    for mode in ("natural", "uniform", "briggs"):
        w, st, D = weights_ref.weights(N, lam, u, v, mode, s=s)
        assert list(st[5:]) == [3.0, 3.0, 2.0], mode
        assert all(w[k] == 0.0 and not np.signbit(w[k]) for k in (3, 6, 7)), mode
        assert w[4] == 5.0 and w[5] == 6.0, mode
        assert D[11] == 6.0 and D.sum() == 9.0 and st[2] == 9.0, mode  # the flagged ones in cell 11 add nothing
    # a taper on a NaN coordinate outside the grid: s t is NaN, and it stays out of the sums
    w, st, D = weights_ref.weights(N, lam, u, v, "uniform", sigma=50.0, s=s)
    assert np.isnan(w[5]) and np.isfinite(st[:4]).all()
    # nothing in the grid: f^2 is 0, noise NaN
    w, st, D = weights_ref.weights(N, lam, [100.0], [0.0], "briggs")
    assert list(w) == [1.0] and st[4] == 0.0 and np.isnan(st[3]) and list(st[5:]) == [0.0, 0.0, 1.0]
    w, st, D = weights_ref.weights(N, lam, [], [], "uniform")
    assert len(w) == 0 and np.isnan(st[3]) and list(st[5:]) == [0.0, 0.0, 0.0]


def test_noise_is_one_for_natural_and_above_otherwise():
    N, lam, u, v, s = scattered()
    for sw in (None, s):
        assert abs(weights_ref.weights(N, lam, u, v, "natural", s=sw)[1][3] - 1.0) < 1e-14
        for mode, R, sig in (("uniform", 0, 0), ("briggs", 0.0, 0), ("briggs", -1.0, 0), ("natural", 0, 40.0),
                             ("uniform", 0, 40.0)):
            assert weights_ref.weights(N, lam, u, v, mode, R, sig, sw)[1][3] > 1.0 + 1e-6, (mode, R, sig)


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


n = 6


def test_context_weights_host_form(rig):
    ctx, rec, run = rig
    u = (np.arange(n, dtype=np.float32) - 2) * 10            # float32: converted
    v = (np.arange(2 * n, dtype=f64) * 3)[::2]               # non-contiguous: converted
    ow, os_ = Out(f64, n), Out(f64, 8)
    w, st = run(lambda: ctx.weights(THETA, LAM, (u, v, None)), "gridhip_weights", THETA, LAM, n, Arr(u, f64), Arr(v, f64), 1,
                None, 1, 0.0, 0.0, ow, os_)
    assert ow.returned(w, (n,)) and os_.returned(st, (8,))
    wt32 = np.arange(n, dtype=np.float32)
    for name, mode in (("natural", 0), ("uniform", 1), ("briggs", 2)):
        ow, os_ = Out(f64, n), Out(f64, 8)
        w, st = run(lambda: ctx.weights(THETA, LAM, (u, v), name, robust=-0.5, taper=120, weights=wt32), "gridhip_weights",
                    THETA, LAM, n, Arr(u, f64), Arr(v, f64), 1, Arr(wt32, f64), mode, -0.5, 120.0, ow, os_)
        assert ow.returned(w, (n,)) and os_.returned(st, (8,))
    # an (n, 3) matrix: views at stride 3; right-form arrays go by their own address; out = weights: in place
    m = np.arange(3 * n, dtype=f64).reshape(n, 3)
    wt = np.ones(n)
    os_ = Out(f64, 8)
    w, st = run(lambda: ctx.weights(THETA, LAM, m, mode="briggs", robust=2, weights=wt, out=wt), "gridhip_weights", THETA,
                LAM, n, Same(m), Same(m, 8), 3, Same(wt), 2, 2.0, 0.0, Same(wt), os_)
    assert w is wt and os_.returned(st, (8,))
    mine = np.zeros(n)
    w, st = run(lambda: ctx.weights(THETA, LAM, m, out=mine), "gridhip_weights", THETA, LAM, n, Same(m), Same(m, 8), 3, None,
                1, 0.0, 0.0, Same(mine), Out(f64, 8))
    assert w is mine


def test_context_weights_refusals_come_before_any_call(rig):
    ctx, rec, run = rig
    u, v = np.zeros(n), np.zeros(n)
    bad = [
        lambda: ctx.weights(THETA, LAM, (u, v), "robust"),                       # not a mode's name
        lambda: ctx.weights(THETA, LAM, (u, v), 1),
        lambda: ctx.weights(THETA, LAM, (u, v), "briggs", robust=float("nan")),
        lambda: ctx.weights(THETA, LAM, (u, v), "briggs", robust=float("inf")),
        lambda: ctx.weights(THETA, LAM, (u, v), taper=-1.0),
        lambda: ctx.weights(THETA, LAM, (u, v), taper=float("nan")),
        lambda: ctx.weights(THETA, LAM, (u, v), weights=np.ones(n + 1)),         # one value per visibility
        lambda: ctx.weights(THETA, LAM, (u, v), weights=np.ones((n, 1))),
        lambda: ctx.weights(THETA, LAM, (u, v), out=np.zeros(n, dtype=np.float32)),  # written in place: no conversion
        lambda: ctx.weights(THETA, LAM, (u, v), out=np.zeros(2 * n)[::2]),
        lambda: ctx.weights(THETA, LAM, (u, v), out=np.zeros(n - 1)),
        lambda: ctx.weights(THETA, LAM, (u, v), out=[0.0] * n),
        lambda: ctx.weights(THETA, LAM, np.zeros((n, 2))),                       # neither a tuple nor (n, 3)
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
    """the argument is the address of the caller's own tensor (+ offset bytes)"""

    def __init__(self, t, offset=0):
        self.t, self.offset = t, offset

    def check(self, arg, where):
        assert address(arg) == self.t.data_ptr() + self.offset, f"{where}: not the caller's tensor"


def tensor_returned(out, t, shape):
    import torch
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == tuple(shape)
    assert t.is_contiguous() and np.array_equal(t.numpy().ravel(), out.fill)
    return True


def test_context_weights_device_form(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    u, v = torch.arange(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    ow, os_ = Out(f64, n), Out(f64, 8)
    w, st = run(lambda: ctx.weights(THETA, LAM, (u, v), "briggs", 0.5, 30.0), "gridhip_weights_dev", THETA, LAM, n, SameT(u),
                SameT(v), 1, None, 2, 0.5, 30.0, ow, os_)
    assert tensor_returned(ow, w, (n,)) and tensor_returned(os_, st, (8,)) and bound == [ctx]
    m = torch.zeros((n, 3), dtype=torch.float64)
    wt = torch.ones(n, dtype=torch.float64)
    w, st = run(lambda: ctx.weights(THETA, LAM, m, "natural", weights=wt, out=wt), "gridhip_weights_dev", THETA, LAM, n,
                SameT(m), SameT(m, 8), 3, SameT(wt), 0, 0.0, 0.0, SameT(wt), Out(f64, 8))
    assert w is wt
    before = len(rec.calls)
    for call in (lambda: ctx.weights(THETA, LAM, (u, v), out=np.zeros(n)),               # a numpy output for tensors
                 lambda: ctx.weights(THETA, LAM, (u, v), weights=np.ones(n)),
                 lambda: ctx.weights(THETA, LAM, (u, v), out=torch.zeros(n, dtype=torch.float32)),
                 lambda: ctx.weights(THETA, LAM, (u, v), weights=torch.ones(n + 1, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before


def test_imager_creation_with_a_weighting(torch_rig):
    """the default creation is the call it was; anything else is the weighted one, with the four arguments before the
    handle's address"""
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    u, v, w = (torch.arange(n, dtype=torch.float64) + k for k in range(3))
    wt = torch.ones(n, dtype=torch.float64)
    hp = Ref(C.c_void_p, 0xABCD)
    head = [0, 0, 0, 0, 0, 0, None, THETA, LAM, n, SameT(u), SameT(v), SameT(w), 1]
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",)), "gridhip_imager_create_dev", *head, hp)
    assert made.n == n and made.N == NPIX
    made._h = None
    for kw, tail in (({"weighting": "natural"}, [0, 0.0, 0.0, None]),
                     ({"weighting": "briggs", "robust": -1, "taper": 75}, [2, -1.0, 75.0, None]),
                     ({"weights": wt}, [1, 0.0, 0.0, SameT(wt)]),
                     ({"taper": 10.0}, [1, 0.0, 10.0, None]),
                     ({"weighting": "briggs", "robust": 0.5, "weights": wt}, [2, 0.5, 0.0, SameT(wt)])):
        made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), **kw), "gridhip_imager_create_weighted_dev", *head,
                   *tail, hp)
        made._h = None
    ko = {"wstep": 40, "qpx": 2, "npixFF": 8, "npixKern": 5}
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("w_cache", ko), weighting="natural"),
               "gridhip_imager_create_weighted_dev", 2, 40, 2, 8, 5, 5, None, *head[7:], 0, 0.0, 0.0, None, hp)
    made._h = None
    wk = torch.zeros((2, 2, 2, 5, 5), dtype=torch.complex128)
    wv = torch.tensor([-10.0, 30.0], dtype=torch.float64)
    ak = torch.zeros((3, 5, 5), dtype=torch.complex128)
    a1, a2 = torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64)
    aw = [THETA, LAM, 2, 2, 5, 3, SameT(wk), SameT(wv), SameT(ak), n, SameT(u), SameT(v), SameT(w), 1, SameT(a1), SameT(a2)]
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("aw", wk, wv, ak), a1, a2), "gridhip_imager_create_aw_dev", *aw, hp)
    made._h = None
    made = run(lambda: ctx.imager(THETA, LAM, (u, v, w), ("aw", wk, wv, ak), a1, a2, weighting="briggs", robust=1.5,
                                  weights=wt), "gridhip_imager_create_aw_weighted_dev", *aw, 2, 1.5, 0.0, SameT(wt), hp)
    made._h = None
    before = len(rec.calls)
    for call in (lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), weighting="superuniform"),
                 lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), weighting="briggs", robust=float("nan")),
                 lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), taper=-2.0),
                 lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), weights=wt[:-1].contiguous()),
                 lambda: ctx.imager(THETA, LAM, (u, v, w), ("simple",), weights=np.ones(n))):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before


def test_imager_weight_stats(torch_rig):
    ctx, im, rec, run, bound, be = torch_rig
    os_ = Out(f64, 8)
    st = run(lambda: im.weight_stats(), "gridhip_imager_weight_stats_dev", os_, handle=im._h)
    assert tensor_returned(os_, st, (8,)) and bound == [ctx]
