"""Time-frequency flagging (gridhip_sumthreshold[_dev], gridhip_sumthreshold_tile), the checks that need no GPU: the
library, the header, the ctypes table and both bindings carry the three entry points; the header states the semantics; a
NULL context is refused whatever else is passed; Context.sumthreshold hands the ABI the right pointers, scalar order and
NULLs and refuses wrong shapes and scalars before any call; waterfall_layout on a hand case; the numpy restatement the GPU
tests compare with (tests/sumthreshold_ref.py) on cubes whose answer is written out by hand; and the quality of the
definition with its default settings on a cube of noise plus interference - a condition on the defaults, checked on the
restatement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sumthreshold_ref as R
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same

NAMES = ["gridhip_sumthreshold", "gridhip_sumthreshold_dev", "gridhip_sumthreshold_tile"]
f64, c128, i64, u8 = np.float64, np.complex128, np.int64, np.uint8
NAN, INF = np.nan, np.inf


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
    assert _lib.SIGNATURES["gridhip_sumthreshold"] == _lib.SIGNATURES["gridhip_sumthreshold_dev"]


def test_header_states_the_semantics():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("time-frequency flagging"):raw.index("int gridhip_sumthreshold(")]
    for phrase in ("[B][T][F]", "[T][B][F]", "FLAGGED ON INPUT", "NOT FINITE", "16 + 8 r + k", "KEPT", "SIR",   # the classes
                   "1.4826", "levels[k] * sigma_b", "M = 2^k", "S^(2m)_j = S^(m)_j + S^(m)_{j+m}", "C_j > 0",
                   "S_j > chi_k * (double)C_j", "M > L", "rint(eta * 2^20)", "q - 2^20", "max_{j > x} P_j - min_{i <= x} P_i >= 0",
                   "+Inf", "{ 0, NaN, NaN, +Inf }", "GRIDHIP_EUNSUPPORTED", "2^18", "2^20", "2^32 - 1",
                   "DETERMINISM", "no floating-point atomic", "both orders", "NOT HERE", "two-sided", "windows above 64"):
        assert phrase in section, phrase
    # residual flagging's section is as it was: the clip's semantics have not moved
    clip = raw[raw.index("residual flagging"):raw.index("int gridhip_flag_residuals(")]
    assert "T_g = med_g + nsigma * sigma_g" in clip and "3 + 33 niter" in clip


def test_bindings_carry_the_three():
    import gridhip
    assert callable(gridhip.Context.sumthreshold) and callable(gridhip.sumthreshold_tile) and callable(gridhip.waterfall_layout)
    assert "sumthreshold_tile" in gridhip.__all__ and "waterfall_layout" in gridhip.__all__
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in doc, name


def test_the_tile():
    import gridhip
    tt, tf = gridhip.sumthreshold_tile()
    assert tt >= 1 and tf >= 1 and tt * tf >= 256  # (a work-group's worth of samples)
    from gridhip import _lib
    lib = _lib.load()
    one = C.c_int64(7)
    assert lib.gridhip_sumthreshold_tile(None, C.byref(one)) == _lib.EINVAL
    assert lib.gridhip_sumthreshold_tile(C.byref(one), None) == _lib.EINVAL and one.value == 7


def test_null_handles_are_refused_and_nothing_is_touched():
    """Without a device no context exists: the argument rules themselves are checked on the GPU
    (test_gpu_sumthreshold.py::test_refusals); here a NULL context is GRIDHIP_EINVAL for good and bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    B, T, Fq = 2, 3, 4
    n = B * T * Fq
    vis, mod, wt = np.full(n, 1 + 2j), np.full(n, 3 + 0j), np.full(n, 4.0)
    wo, fl, bs, st = np.full(n, 8.0), np.full(n, 9, dtype=u8), np.full((B, 4), 5.0), np.full(8, 6.0)
    lv = np.array([6.0, 4.0])
    pv, pm, pw, pwo, pf, pbs, pst = (C.c_void_p(a.ctypes.data) for a in (vis, mod, wt, wo, fl, bs, st))
    pl = lv.ctypes.data_as(C.POINTER(C.c_double))
    cases = [(B, T, Fq, 0, 2, pl, 0.2, 0.2, 8, 2), (B, T, Fq, 1, 1, pl, 0.0, 0.0, 1, 0), (0, T, Fq, 0, 2, pl, 0.2, 0.2, 8, 2),
             (B, T, Fq, 2, 2, pl, 0.2, 0.2, 8, 2), (B, T, Fq, 0, 0, pl, 0.2, 0.2, 8, 2), (B, T, Fq, 0, 8, pl, 0.2, 0.2, 8, 2),
             (B, T, Fq, 0, 2, None, 0.2, 0.2, 8, 2), (B, T, Fq, 0, 2, pl, 1.0, 0.2, 8, 2), (B, T, Fq, 0, 2, pl, 0.2, -0.1, 8, 2),
             (B, T, Fq, 0, 2, pl, 0.2, 0.2, 0, 2), (B, T, Fq, 0, 2, pl, 0.2, 0.2, 8, 5), ((1 << 18) + 1, 1, 1, 0, 2, pl, 0.2, 0.2, 8, 2)]
    for fn in (lib.gridhip_sumthreshold, lib.gridhip_sumthreshold_dev):
        for (b, t, f, order, K, levels, ef, et, mc, niter) in cases:
            assert fn(None, b, t, f, order, pv, pm, pw, K, levels, ef, et, mc, niter, pwo, pf, pbs, pst) == _lib.EINVAL
            assert fn(None, b, t, f, order, pv, None, None, K, levels, ef, et, mc, niter, pwo, None, None, None) == _lib.EINVAL
        assert fn(None, B, T, Fq, 0, None, pm, pw, 2, pl, 0.2, 0.2, 8, 2, None, pf, pbs, pst) == _lib.EINVAL
        assert fn(None, B, T, Fq, 0, pv, pm, pw, 2, pl, 0.2, 0.2, 8, 2, pv, pf, pbs, pst) == _lib.EINVAL   # wt_out over vis
    for a, val in ((vis, 1 + 2j), (mod, 3 + 0j), (wt, 4.0), (wo, 8.0), (fl, 9), (bs, 5.0), (st, 6.0)):
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


class Levels:
    """the argument is a double pointer to these thresholds"""

    def __init__(self, values):
        self.want = np.array(values, dtype=f64)

    def check(self, arg, where):
        assert isinstance(arg, C.POINTER(C.c_double)), where
        got = np.array([arg[i] for i in range(len(self.want))])
        assert np.array_equal(got, self.want), f"{where}: {got} != {self.want}"


SHAPE = (2, 3, 4)
NS = 24


def test_sumthreshold_marshalling(rig):
    ctx, rec, run = rig
    vis = (np.arange(NS) * (1 - 0.5j)).astype(np.complex64).reshape(SHAPE)
    mod = (np.arange(2 * NS) + 1j).astype(c128)[::2].reshape(SHAPE)  # not contiguous
    wt = np.arange(NS, dtype=np.float32).reshape(SHAPE)
    assert not mod.flags.c_contiguous
    w, f, b, s = Out(f64, NS), Out(u8, NS), Out(f64, 2 * 4), Out(f64, 8)
    got = run(lambda: ctx.sumthreshold(vis, mod, wt, levels=[5, 3], eta=(0.25, 0), min_count=3, niter=4),
              "gridhip_sumthreshold", 2, 3, 4, 0, Arr(vis, c128), Arr(mod, c128), Arr(wt, f64), 2, Levels([5.0, 3.0]), 0.25, 0.0,
              3, 4, w, f, b, s)
    assert w.returned(got[0], SHAPE) and f.returned(got[1], SHAPE) and b.returned(got[2], (2, 4)) and s.returned(got[3], (8,))
    # order "tbf": the cube is [T][B][F], B is its second axis; model_vis and weights None are NULL; the defaults are the
    # ladder 6 / 1.5^k of 7 stages, eta (0.2, 0.2), min_count 8, niter 2; an array in the ABI's form goes by its own address
    v2 = np.ascontiguousarray(vis, dtype=c128)
    got = run(lambda: ctx.sumthreshold(v2, order="tbf"), "gridhip_sumthreshold", 3, 2, 4, 1, Same(v2), None, None, 7,
              Levels([6.0 / 1.5 ** k for k in range(7)]), 0.2, 0.2, 8, 2, Out(f64, NS), Out(u8, NS), Out(f64, 12), Out(f64, 8))
    assert got[0].shape == SHAPE and got[1].shape == SHAPE and got[1].dtype == u8 and got[2].shape == (3, 4)
    got = run(lambda: ctx.sumthreshold(v2, nsigma=8, rho=2, nlevels=3), "gridhip_sumthreshold", 2, 3, 4, 0, Same(v2), None, None, 3,
              Levels([8.0, 4.0, 2.0]), 0.2, 0.2, 8, 2, Out(f64, NS), Out(u8, NS), Out(f64, 8), Out(f64, 8))
    # in place: out may be the weights themselves, and is what comes back
    w2 = np.ones(SHAPE)
    got = run(lambda: ctx.sumthreshold(v2, weights=w2, out=w2, niter=0), "gridhip_sumthreshold", 2, 3, 4, 0, Same(v2), None,
              Same(w2), 7, Levels(R.ladder()), 0.2, 0.2, 8, 0, Same(w2), Out(u8, NS), Out(f64, 8), Out(f64, 8))
    assert got[0] is w2


def test_wrong_shapes_and_scalars_are_refused_before_any_call(rig):
    ctx, rec, run = rig
    vis = np.zeros(SHAPE, dtype=c128)
    bad = [dict(vis=np.zeros(NS, dtype=c128)), dict(vis=np.zeros((2, 3, 0), dtype=c128)), dict(model_vis=vis[:, :, :-1]),
           dict(weights=np.ones((3, 2, 4))), dict(weights=np.ones(SHAPE, dtype=c128)), dict(order="fbt"), dict(levels=[]),
           dict(levels=[1.0] * 8), dict(levels=[6.0, 0.0]), dict(levels=[6.0, -1.0]), dict(levels=[np.inf]), dict(levels=[np.nan]),
           dict(nsigma=0.0), dict(nsigma=np.inf), dict(rho=0.0), dict(nlevels=0), dict(nlevels=8), dict(eta=(1.0, 0.2)),
           dict(eta=(0.2, -0.1)), dict(eta=(np.nan, 0.2)), dict(eta=(0.2,)), dict(min_count=0), dict(niter=-1), dict(niter=5),
           dict(out=np.zeros(SHAPE, dtype=np.float32)), dict(out=np.zeros(NS)), dict(out=np.zeros((2, 3, 8))[:, :, ::2])]
    for change in bad:
        with pytest.raises(ValueError):
            ctx.sumthreshold(**{**dict(vis=vis), **change})
    assert rec.calls == []


# ---- waterfall_layout ----------------------------------------------------------------------------------------------------
def test_waterfall_layout_on_a_hand_case():
    import torch
    import gridhip
    a1, a2 = [0, 1, 0, 2], [1, 0, 2, 0]     # the unordered pairs (0,1) (0,1) (0,2) (0,2): baselines 0 0 1 1
    time, chan = [0, 1, 1, 0], [0, 1, 2, 0]
    index, B, pairs = gridhip.waterfall_layout(a1, a2, time, 2, chan, 3)
    assert B == 2 and pairs.tolist() == [[0, 1], [0, 2]] and index.dtype == torch.int64
    assert index.tolist() == [0, 4, 11, 6]       # ((b * 2 + t) * 3 + c)
    index_t, B, _ = gridhip.waterfall_layout(a1, a2, time, 2, chan, 3, order="tbf")
    assert index_t.tolist() == [0, 7, 11, 3]     # ((t * 2 + b) * 3 + c)
    # the way in and the way back; the cells nobody fills keep the weight 0
    stream = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    for idx, shape in ((index, (2, 2, 3)), (index_t, (2, 2, 3))):
        cube = torch.zeros(shape, dtype=torch.float64)
        cube.view(-1)[idx] = stream
        assert int((cube == 0).sum()) == 8 and cube.view(-1)[idx].tolist() == stream.tolist()
    both = torch.zeros((2, 2, 3)), torch.zeros((2, 2, 3))
    both[0].view(-1)[index], both[1].view(-1)[index_t] = stream.float(), stream.float()
    assert torch.equal(both[0], both[1].transpose(0, 1))  # the same cube in the two orders
    for kw in (dict(order="fbt"), dict(time=[0, 2, 1, 0]), dict(chan=[0, 1, 3, 0]), dict(time=[0, -1, 1, 0]), dict(a2=[1, 0, 2])):
        with pytest.raises(ValueError):
            gridhip.waterfall_layout(**{**dict(a1=a1, a2=a2, time=time, ntime=2, chan=chan, nchan=3), **kw})
    index, B, pairs = gridhip.waterfall_layout([], [], [], 2, [], 3)
    assert index.numel() == 0 and B == 1


# ---- the restatement on cubes worked by hand -------------------------------------------------------------------------------
ROW = [10, 12, 8, 10, 16, 16, 9, 11]  # sorted 8 9 10 10 11 12 16 16: the lower median is 10; |a - 10| sorted 0 0 1 1 2 2 6 6: MAD 1
SIGMA = 1.4826


def test_two_adjacent_samples_that_only_stage_1_catches():
    """e = 0 2 -2 0 6 6 -1 1.  Stage 0, chi = 5 sigma = 7.4: no sample.  Stage 1, chi = 3.5 sigma = 5.19: the pairs sum to
    2 0 -2 6 12 5 0 against 2 chi = 10.4 - window 4 alone, the samples 4 and 5.  Round 1: 10 12 8 10 9 11, median 10, MAD 1
    again; with x = 0 for the two flagged the pairs sum to 2 0 -2 0 0 -1 0 and nothing is hit: two rounds run."""
    vis = np.array(ROW, dtype=c128).reshape(1, 1, 8)
    w, f, b, s = R.sumthreshold(vis, levels=[5.0, 3.5], eta=(0, 0), min_count=4, niter=3)
    assert f.tolist() == [[[0, 0, 0, 0, 17, 17, 0, 0]]] and w.tolist() == [[[1, 1, 1, 1, 0, 0, 1, 1]]]
    assert b.tolist() == [[6, 10.0, 1.0, 5.0 * SIGMA]] and s.tolist() == [2, 8, 2, 0, 0, 0, 0, 6]
    # one stage: nothing; niter = 1: the statistics round 0 saw
    w, f, b, s = R.sumthreshold(vis, levels=[5.0], eta=(0, 0), min_count=4, niter=3)
    assert not f.any() and s.tolist() == [1, 8, 0, 0, 0, 0, 0, 8]
    w, f, b, s = R.sumthreshold(vis, levels=[5.0, 3.5], eta=(0, 0), min_count=4, niter=1)
    assert b.tolist() == [[8, 10.0, 1.0, 5.0 * SIGMA]] and s.tolist() == [1, 8, 2, 0, 0, 0, 0, 6]
    # the same row along time
    w, f, b, s = R.sumthreshold(vis.reshape(1, 8, 1), levels=[5.0, 3.5], eta=(0, 0), min_count=4, niter=3)
    assert f.ravel().tolist() == [0, 0, 0, 0, 17, 17, 0, 0]
    # below min_count, or a baseline of ties: not thresholded, chi_0 = +Inf
    w, f, b, s = R.sumthreshold(vis, levels=[5.0, 3.5], eta=(0, 0), min_count=9, niter=3)
    assert not f.any() and b.tolist() == [[8, 10.0, 1.0, INF]] and s[0] == 1
    w, f, b, s = R.sumthreshold(np.full((1, 2, 4), 3 + 4j), levels=[5.0, 3.5], eta=(0, 0), min_count=1, niter=3)
    assert not f.any() and b.tolist() == [[8, 5.0, 0.0, INF]]


def test_a_flagged_sample_inside_a_window_is_left_out_of_sum_and_count():
    """The row with a sample of amplitude 1000 and weight 0 between the two 16s: the statistics are the row's.  Stage 1: the
    windows {16, flagged} hold one participant, S = 6 against chi * 1 = 5.19 - hit, twice; had the flagged sample counted,
    6 against 2 chi = 10.4 would not be.  The flagged sample keeps its code 1."""
    a = ROW[:5] + [1000] + ROW[5:]
    wt = np.ones(9)
    wt[5] = 0.0
    w, f, b, s = R.sumthreshold(np.array(a, dtype=c128).reshape(1, 1, 9), weights=wt.reshape(1, 1, 9), levels=[5.0, 3.5],
                                eta=(0, 0), min_count=4, niter=3)
    assert f.ravel().tolist() == [0, 0, 0, 0, 17, 1, 17, 0, 0] and s.tolist() == [2, 8, 2, 0, 0, 0, 1, 6]
    assert w.ravel().tolist() == [1, 1, 1, 1, 0, 0, 0, 1, 1] and not np.signbit(w).any()


def test_a_window_longer_than_the_row_does_nothing():
    """1 2 4: median 2, MAD 1.  The third level is tiny, but its window of 4 fits neither the 3 channels nor the 1 time step.
    1 2 4 3: median 2, MAD 1, e sums to 2 > 4 * 0.001 sigma - the one window flags all four, and round 1 meets an empty
    baseline."""
    lv = [100.0, 100.0, 0.001]
    w, f, b, s = R.sumthreshold(np.array([1, 2, 4], dtype=c128).reshape(1, 1, 3), levels=lv, eta=(0, 0), min_count=1, niter=2)
    assert not f.any() and b.tolist() == [[3, 2.0, 1.0, 100.0 * SIGMA]] and s.tolist() == [1, 3, 0, 0, 0, 0, 0, 3]
    w, f, b, s = R.sumthreshold(np.array([1, 2, 4, 3], dtype=c128).reshape(1, 1, 4), levels=lv, eta=(0, 0), min_count=1, niter=2)
    assert f.ravel().tolist() == [18] * 4 and s.tolist() == [2, 4, 4, 0, 0, 0, 0, 0]
    assert b[0, 0] == 0 and np.isnan(b[0, 1:3]).all() and b[0, 3] == INF
    w, f, b, s = R.sumthreshold(np.array([1, 2, 4, 3], dtype=c128).reshape(1, 4, 1), levels=lv, eta=(0, 0), min_count=1, niter=1)
    assert f.ravel().tolist() == [18] * 4 and b.tolist() == [[4, 2.0, 1.0, 100.0 * SIGMA]]


def test_the_threshold_is_strict():
    """0 0 0 1 1 1 2 2 x: median 1, MAD 1, chi = 2 sigma = 2.9652.  x = 1 + chi is exact (both lie in [2, 4)), so e = chi to
    the bit: a sample exactly at chi is not above it, the next double is."""
    a = np.array([0, 0, 0, 1, 1, 1, 2, 2, 0], dtype=f64)
    level = 2.0
    chi = level * (1.4826 * 1.0)
    a[-1] = 1.0 + chi
    assert (a[-1] - 1.0) == chi
    w, f, b, s = R.sumthreshold(a.astype(c128).reshape(1, 1, 9), levels=[level], eta=(0, 0), min_count=1, niter=1)
    assert not f.any()
    a[-1] = np.nextafter(a[-1], INF)
    w, f, b, s = R.sumthreshold(a.astype(c128).reshape(1, 1, 9), levels=[level], eta=(0, 0), min_count=1, niter=1)
    assert f.ravel().tolist() == [0] * 8 + [16]


def sir(codes, eta):
    c = np.array(codes, dtype=u8).reshape(1, -1)
    R.sir_rows(c, eta)
    return c.ravel().tolist()


def test_sir_closes_a_gap_when_eta_allows():
    """0 F F 0 F F 0.  The middle sample sits in F F 0 F F: 4 q + (q - 2^20) >= 0 needs q >= 209715.2 - eta = 0.2 gives
    q = 209715 and does not close it, 0.21 does.  The ends need 2 q + (q - 2^20) >= 0, eta >= 1/3."""
    row = [0, 16, 16, 0, 16, 16, 0]
    assert sir(row, 0.0) == row and sir(row, 0.19) == row and sir(row, 0.2) == row
    assert sir(row, 0.21) == [0, 16, 16, 8, 16, 16, 0] and sir(row, 0.33) == [0, 16, 16, 8, 16, 16, 0]
    assert sir(row, 0.34) == [8, 16, 16, 8, 16, 16, 8]
    assert sir([0] * 7, 0.9) == [0] * 7 and sir([16, 3, 8], 0.5) == [16, 3, 8] and sir([0], 0.9) == [0] and sir([3], 0.5) == [3]


def test_sir_across_a_gap_of_missing_cells():
    """F F 1 1 1 0 F F: the missing cells weigh nothing, so the sample sees F F 0 F F as before and 0.21 flags it; with
    kept samples in their place it sees 0 0 0 0 F F, and its best interval 0 F F needs 1/3."""
    assert sir([16, 16, 1, 1, 1, 0, 16, 16], 0.19) == [16, 16, 1, 1, 1, 0, 16, 16]
    assert sir([16, 16, 1, 1, 1, 0, 16, 16], 0.21) == [16, 16, 1, 1, 1, 8, 16, 16]
    assert sir([16, 16, 0, 0, 0, 0, 16, 16], 0.21) == [16, 16, 0, 0, 0, 0, 16, 16]
    assert sir([16, 16, 0, 0, 0, 0, 16, 16], 0.34) == [16, 16, 8, 0, 0, 8, 16, 16]


def test_sir_runs_without_rounds_along_frequency_then_time():
    vis = np.ones((1, 1, 7), dtype=c128)
    vis[0, 0, [1, 2, 4, 5]] = NAN
    w, f, b, s = R.sumthreshold(vis, eta=(0.21, 0.0), niter=0)
    assert f.ravel().tolist() == [0, 3, 3, 8, 3, 3, 0] and s.tolist() == [0, 3, 0, 4, 1, 0, 0, 2]
    assert b.tolist()[0][0] == 3 and np.isnan(b[0, 1:3]).all() and b[0, 3] == INF
    w, f, b, s = R.sumthreshold(vis, eta=(0.0, 0.21), niter=0)       # (along time the row is one sample long)
    assert f.ravel().tolist() == [0, 3, 3, 0, 3, 3, 0]
    w, f, b, s = R.sumthreshold(vis.reshape(1, 7, 1), eta=(0.0, 0.21), niter=0)
    assert f.ravel().tolist() == [0, 3, 3, 8, 3, 3, 0]
    # the time pass works on the result of the frequency pass: the 8 of row 1 closes the column 0 8 8 . 8 8 0
    cube = np.ones((1, 7, 7), dtype=c128)
    for t in (1, 2, 4, 5):
        cube[0, t, [1, 2, 4, 5]] = NAN
    w, f, b, s = R.sumthreshold(cube, eta=(0.21, 0.21), niter=0)
    assert f[0, 1].tolist() == [0, 3, 3, 8, 3, 3, 0] and f[0, 3].tolist() == [0, 8, 8, 8, 8, 8, 0] and f[0, 0].tolist() == [0] * 7
    assert s[4] == 4 + 5


# ---- the quality of the definition, with the defaults -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_defaults_find_the_interference_and_keep_the_noise(seed):
    """(4, 96, 160) of unit complex Gaussian noise; +1.5 on four time steps of baseline 1, +1.0 on channel 50 of baseline 2,
    +12 on one sample of baseline 3, channel 100 of baseline 0 flagged on input.  The defaults, niter = 2.  Required: at
    least 0.99 of the injected samples flagged before SIR; of the rest at most 0.012 before SIR and 0.02 after it."""
    vis, wt, injected = R.interference_cube(seed)
    pre = []
    w, f, b, s = R.sumthreshold(vis, weights=wt, before_sir=pre)
    rest = ~injected & (wt > 0)
    found, false_pre, false_post = (pre[0][injected] >= 16).mean(), (pre[0][rest] >= 16).mean(), (f[rest] != 0).mean()
    print(f"seed {seed}: injected found {found:.4f}; rest flagged before SIR {false_pre:.4f}, after {false_post:.4f}; stats {s}")
    assert found >= 0.99 and false_pre <= 0.012 and false_post <= 0.02
    assert (f[0, :, 100] == 1).all() and f[3, 40, 70] >= 16 and s[6] == 96
