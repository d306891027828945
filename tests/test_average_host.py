"""Phase shift and averaging (gridhip_phase_shift[_dev], gridhip_average[_dev]), the checks that need no GPU: the library,
the header, the ctypes table and the Python surface carry the four entry points; the header states the rules; a NULL
context is refused whatever else is passed and the binding refuses wrong shapes before any call; the numpy restatement the
GPU tests compare with (tests/average_ref.py) does not depend on the order of the stream and lies within the header's
bound of math.fsum; the rotation helpers and average_groups are right on cases worked by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import average_ref as A
from conftest import ROOT

NAMES = ["gridhip_phase_shift", "gridhip_phase_shift_dev", "gridhip_average", "gridhip_average_dev"]
f64, c128, i64 = np.float64, np.complex128, np.int64


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
    assert _lib.SIGNATURES["gridhip_phase_shift"] == _lib.SIGNATURES["gridhip_phase_shift_dev"]
    assert _lib.SIGNATURES["gridhip_average"] == _lib.SIGNATURES["gridhip_average_dev"]
    # R is the host's in both forms: a typed pointer, not an array the back end takes the address of
    assert _lib.SIGNATURES["gridhip_phase_shift_dev"][1][2] is _lib._HOST_F64
    assert _lib.SIGNATURES["gridhip_average_dev"][1][4] is _lib._HOST_F64
    assert len(_lib.SIGNATURES["gridhip_phase_shift"][1]) == 14 and len(_lib.SIGNATURES["gridhip_average"][1]) == 21
    assert _lib.load().gridhip_version() >= 270
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 270
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in hs, name


def test_header_states_the_rules():
    raw = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = raw[raw.index("phase shift and averaging"):raw.index("int gridhip_phase_shift(")]
    for phrase in ("PHASE RULE", "vis_out = vis_in * exp(+2 pi i p)", "p = u l0 + v m0 + w (n0 - 1)",
                   "n0 - 1 = -r2 / (1 + sqrt(1 - r2))", "r = p - rint(p)", "gridhip_dft_predict", "becomes the constant S",
                   "COORDINATE RULE", "u' = (R00 u + R01 v) + R02 w", "contraction is off", "ALIASING", "vis_out == vis_in",
                   "R22 <= 0", "|R R^T - I| above 1e-9", "HOST doubles",
                   "FLAGGED", "LEFT OUT", "NOT FINITE", "PARTICIPANT", "EXACT INTEGER SUMS", "L = ceil(log2 n_g)",
                   "s = 1084 - L - b", "q = (int64) rint(ldexp(y, s))", "|q| <= 2^(62 - L)", "ldexp((double) Q, -s)",
                   "|sum - exact| <= n_g 2^(L-62) M + 2^-53 |sum|", "M = max(max|y|, 2^-1022)", "wt = +0.0", "DEFINED BY THE CALLS IT REPLACES",
                   "no shifted stream is written", "GRIDHIP_EUNSUPPORTED", "2^31 - 256", "n = 0 is valid",
                   "no memset node", "fixed number of launches", "DETERMINISM", "integer atomics only",
                   "no sum of doubles", "same bits"):
        assert phrase in section, phrase


def test_python_surface():
    import gridhip
    for owner, name in ((gridhip.Context, "phase_shift"), (gridhip.Context, "average"), (gridhip, "rotation_to"),
                        (gridhip, "rotation_radec"), (gridhip, "average_groups")):
        assert callable(getattr(owner, name)), name
    for name in ("rotation_to", "rotation_radec", "average_groups"):
        assert name in gridhip.__all__


def test_null_context_is_refused_and_nothing_is_touched():
    """Without a device no context exists, so the argument rules themselves are checked on the GPU
    (test_gpu_average.py::test_refusals); here: a NULL context is GRIDHIP_EINVAL for good and for bad arguments alike."""
    from gridhip import _lib
    lib = _lib.load()
    n, G = 4, 2
    R = np.eye(3)
    Rp = R.ctypes.data_as(C.POINTER(C.c_double))
    uvw, vis, grp, wt = np.full((n, 3), 2.0), np.full(n, 1 + 2j), np.array([0, 1, 0, 1], dtype=i64), np.full(n, 3.0)
    o3, ov, ow, oc, st = np.full((G, 3), 5.0), np.full(G, 6 + 0j), np.full(G, 7.0), np.full(G, 8, dtype=i64), np.full(8, 9.0)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)  # noqa: E731
    cols, ocols = (p(uvw), p(uvw, 8), p(uvw, 16)), (p(o3), p(o3, 8), p(o3, 16))
    for fn in (lib.gridhip_phase_shift, lib.gridhip_phase_shift_dev):
        for nn, RR in ((n, Rp), (-1, Rp), (n, None), (0, Rp)):
            assert fn(None, nn, RR, *cols, 3, p(vis), p(vis), *cols, 3, p(st)) == _lib.EINVAL
            assert fn(None, nn, RR, *cols, 3, p(vis), p(vis), None, None, None, 3, None) == _lib.EINVAL
    for fn in (lib.gridhip_average, lib.gridhip_average_dev):
        for nn, GG, RR in ((n, G, None), (n, G, Rp), (-1, G, None), (n, 0, None), (n, 1 << 40, None)):
            assert fn(None, nn, GG, p(grp), RR, *cols, 3, None, p(vis), p(wt), *ocols, 3, None, p(ov), p(ow), p(oc),
                      p(st)) == _lib.EINVAL
    for a, val in ((uvw, 2.0), (vis, 1 + 2j), (wt, 3.0), (o3, 5.0), (ov, 6 + 0j), (ow, 7.0), (oc, 8), (st, 9.0)):
        assert np.all(a == val)


class _NoCalls:
    """stands in for the loaded library: any entry point that is reached is an error"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_the_binding_refuses_before_any_call():
    import gridhip
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = _NoCalls(), C.c_void_p(1), 0
    try:
        n = 5
        uvw, vis, grp, R = np.zeros((n, 3)), np.zeros(n, dtype=c128), np.zeros(n, dtype=i64), np.eye(3)
        bad_shift = [dict(vis=vis[:-1]), dict(R=None), dict(R=np.eye(4)), dict(uvw=np.zeros((n, 2))),
                     dict(out=np.zeros(n, dtype=np.complex64)), dict(out=np.zeros(n + 1, dtype=c128))]
        for change in bad_shift:
            with pytest.raises(ValueError):
                ctx.phase_shift(**{**dict(uvw=uvw, vis=vis, R=R), **change})
        bad_avg = [dict(vis=vis[:-1]), dict(group=grp[:-1]), dict(group=grp.astype(f64)), dict(G=None), dict(G=0),
                   dict(group=None, G=2), dict(weights=np.ones(n - 1)), dict(weights=np.ones(n, dtype=c128)),
                   dict(x=np.ones(n + 1)), dict(R=np.eye(2))]
        for change in bad_avg:
            with pytest.raises(ValueError):
                ctx.average(**{**dict(uvw=uvw, vis=vis, group=grp, G=1), **change})
    finally:
        ctx._h = None


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
def _stream(rng, n, G):
    grp = rng.integers(-1, G + 1, n)
    u, v, w = rng.normal(size=(3, n)) * 1e3
    vis = (rng.normal(size=n) + 1j * rng.normal(size=n)) * 10.0 ** rng.integers(-5, 6, n)
    wt = rng.uniform(0.1, 2.0, n)
    wt[rng.random(n) < 0.05] = 0.0
    return grp, u, v, w, vis, rng.normal(size=n), wt


def test_reference_is_permutation_invariant():
    rng = np.random.default_rng(1)
    n, G = 2000, 9
    grp, u, v, w, vis, x, wt = _stream(rng, n, G)
    vis[7], wt[11], u[13] = np.inf, np.nan, np.nan
    want = A.average(grp, G, u, v, w, vis, x, wt)
    for seed in (2, 3):
        p = np.random.default_rng(seed).permutation(n)
        got = A.average(grp[p], G, u[p], v[p], w[p], vis[p], x[p], wt[p])
        for a, b in zip(got, want):
            assert A.same_bits(a, b)
    assert want[7].tolist()[1:5] == [(A.classes(grp, G, [wt * vis.real, wt * vis.imag, wt * u, wt * v, wt * w, wt * x], wt)
                                      == c).sum() for c in range(4)]


def _bound(n, L, cols, got):
    """the header's bound: n_g roundings of at most half the quantum 2^-s <= 2^(L-61) M each, M = max|y| but no less than
    the smallest normal 2^-1022 (below it the quantum stays 2^(L-1084)), and the conversion's, half an ulp of the sum -
    and as much again for math.fsum's own rounding of the exact sum, which is what the sum is compared with"""
    M = max(max(np.abs(c).max() for c in cols), 2.0 ** -1022)
    return n * 2.0 ** (L - 62) * M + 2 * 2.0 ** -53 * abs(float(got)) + 5e-324


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1024, 1025])
def test_reference_is_within_the_stated_bound_of_fsum(n):
    rng = np.random.default_rng(n)
    L = A.log2_ceil(n)
    for scale in (1.0, 1e-300, 1e300 / n, 5e-324):
        cols = [rng.normal(size=n) * 10.0 ** rng.integers(-8, 1, n) * scale for _ in range(2)]
        # values of one sign and nearly one size: the sum is n times the largest, and its conversion rounds
        cols.append((1.0 + rng.integers(0, 1 << 20, n) * 2.0 ** -52) * scale)
        sums, s = A.integer_sum(cols)
        big = max(np.abs(c).max() for c in cols)
        for j, (c, got) in enumerate(zip(cols, sums)):
            exact = math.fsum(c.tolist())
            print(f"n {n} scale {scale} column {j}: |sum - exact| {abs(float(got) - exact):.3e}, bound {_bound(n, L, cols, got):.3e}")
            assert abs(float(got) - exact) <= _bound(n, L, cols, got), (n, scale, j)
            if j < 2 and scale != 5e-324:  # mixed signs in the normal range: also the shorter form, with 2^-52 max|y|
                assert abs(float(got) - exact) <= (n * 2.0 ** (L - 62) + 2.0 ** -52) * big, (n, scale, j)


def test_reference_on_edge_groups():
    # all zeros and -0.0: +0.0; denormals: exact; 1e-300 beside 1e300: the small one is below the quantum
    z, _ = A.integer_sum([np.array([0.0, -0.0, 0.0])])
    assert z[0] == 0.0 and not np.signbit(z[0])
    d, s = A.integer_sum([np.array([5e-324, 1e-310, -2e-310])])
    assert s == 1084 - 2 and d[0] == math.fsum([5e-324, 1e-310, -2e-310])
    m, _ = A.integer_sum([np.array([1e-300, 1e300])])
    assert m[0] == 1e300
    # a group without participants: zeros, the weight +0.0, count 0; a fully flagged group is such a group
    r = A.average(np.array([0, 0, 2]), 3, np.ones(3), np.ones(3), np.ones(3), np.ones(3, dtype=c128), None,
                  np.array([0.0, -1.0, 2.0]))
    assert r[6].tolist() == [0, 0, 1] and r[5].tolist() == [0.0, 0.0, 2.0] and not np.signbit(r[5]).any()
    assert r[4].tolist() == [0, 0, 1 + 0j] and r[7].tolist() == [1, 1, 2, 0, 0, 1, 0, 0]
    # the weighted mean on numbers worked by hand: weights 1 and 3, values 2 and 6 -> (2 + 18) / 4 = 5
    r = A.average(None, 1, np.array([2.0, 6.0]), np.zeros(2), np.zeros(2), np.array([2 + 4j, 6 - 4j]), None, np.array([1.0, 3.0]))
    assert r[0][0] == 5.0 and r[4][0] == 5 - 2j and r[5][0] == 4.0 and r[6][0] == 2


def test_reference_phase_shift_on_a_point():
    """a point of flux S at (l0, m0), V = S exp(-2 pi i p), becomes the constant S"""
    import gridhip
    rng = np.random.default_rng(5)
    l0, m0 = 0.03, -0.02
    R = gridhip.rotation_to(l0, m0)
    u, v, w = rng.normal(size=(3, 50)) * 500.0
    p = u * l0 + v * m0 + w * (R[2, 2] - 1.0)
    vis = 2.5 * np.exp(-2j * np.pi * p)
    out, (u1, v1, w1), bad = A.phase_shift(R, u, v, w, vis)
    assert bad == 0 and np.abs(out - 2.5).max() < 1e-9
    assert np.allclose(np.stack([u1, v1, w1]), R @ np.stack([u, v, w]), rtol=0, atol=1e-10)
    u[3] = np.nan
    out, _, bad = A.phase_shift(R, u, v, w, vis)
    assert bad == 1 and out[3] == vis[3]


# ---- the rotation helpers ------------------------------------------------------------------------------------------------
def test_rotation_helpers():
    import gridhip
    for l0, m0 in ((0.0, 0.0), (0.1, -0.2), (-0.6, 0.7), (1e-9, 0.0)):
        R = gridhip.rotation_to(l0, m0)
        assert R.shape == (3, 3) and R.dtype == f64
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert R[2].tolist() == [l0, m0, math.sqrt(1.0 - (l0 * l0 + m0 * m0))]
        # minimal: the axis of the turn, (m0, -l0, 0) normalised, is left alone
        if l0 or m0:
            axis = np.array([m0, -l0, 0.0]) / math.hypot(l0, m0)
            assert np.abs(R @ axis - axis).max() < 1e-14
    assert np.array_equal(gridhip.rotation_to(0, 0), np.eye(3))
    for bad in ((1.0, 0.0), (0.8, 0.8)):
        with pytest.raises(ValueError):
            gridhip.rotation_to(*bad)
    ra0, dec0, ra1, dec1 = 0.3, -0.5, 0.35, -0.45
    R = gridhip.rotation_radec(ra0, dec0, ra1, dec1)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1.0) < 1e-14
    assert abs(R[2, 0] - math.cos(dec1) * math.sin(ra1 - ra0)) < 1e-15
    assert abs(R[2, 1] - (math.sin(dec1) * math.cos(dec0) - math.cos(dec1) * math.sin(dec0) * math.cos(ra1 - ra0))) < 1e-15
    assert abs(R[2, 2] - (math.sin(dec1) * math.sin(dec0) + math.cos(dec1) * math.cos(dec0) * math.cos(ra1 - ra0))) < 1e-15
    assert np.abs(gridhip.rotation_radec(1.1, 0.4, 1.1, 0.4) - np.eye(3)).max() < 1e-15


# ---- average_groups --------------------------------------------------------------------------------------------------------
def _observation():
    """3 antennas (baselines (0,1), (0,2), (1,2)), 8 times, 4 channels; time-major, then baseline, then channel"""
    pairs = [(0, 1), (2, 0), (1, 2)]  # (2, 0): the unordered pair (0, 2)
    a1, a2, t, ch = [], [], [], []
    for ti in range(8):
        for (p, q) in pairs:
            for c in range(4):
                a1.append(p), a2.append(q), t.append(ti), ch.append(c)
    return np.array(a1), np.array(a2), np.array(t), np.array(ch)


def test_average_groups_by_hand():
    import torch
    import gridhip
    a1, a2, t, ch = _observation()
    n = len(a1)
    g, G, g1, g2 = gridhip.average_groups(a1, a2, t)
    assert G == 3 * 8 and g.dtype == torch.int64 and tuple(g.shape) == (n,)
    lo, hi = np.minimum(a1, a2), np.maximum(a1, a2)
    bl = np.array([{(0, 1): 0, (0, 2): 1, (1, 2): 2}[(a, b)] for a, b in zip(lo, hi)])
    assert g.tolist() == (bl * 8 + t).tolist()                      # the sorted keys: pair, then window
    assert g1.tolist() == [0] * 8 + [0] * 8 + [1] * 8 and g2.tolist() == [1] * 8 + [2] * 8 + [2] * 8
    g, G, _, _ = gridhip.average_groups(a1, a2, t, ntime=4, chan=ch, nchan=2)
    assert G == 3 * 2 * 2 and g.tolist() == (bl * 4 + (t // 4) * 2 + ch // 2).tolist()
    g, G, _, _ = gridhip.average_groups(a1, a2, t, ntime=3, chan=ch, nchan=4)   # windows of 3, 3 and 2 times
    assert G == 9 and g.tolist() == (bl * 3 + t // 3).tolist()
    # baseline-dependent: lengths 100, 40, 12.5 -> factors clamp(floor(2 * 100 / L), 2, 8) = 2, 5, 8
    length = np.array([100.0, 40.0, 12.5])[bl]
    uvw = np.stack([0.6 * length, 0.8 * length, np.zeros(n)], axis=1)
    uvw[t == 0] *= 0.5                                             # the LARGEST length of a baseline counts
    g, G, g1, g2 = gridhip.average_groups(a1, a2, t, ntime=2, uvw=uvw, bda=8)
    f = np.array([2, 5, 8])[bl]
    first = np.array([0, 4, 6])[bl]                                # 4 windows, then 2 (5 + 3 times), then 1
    assert G == 7 and g.tolist() == (first + t // f).tolist()
    assert g1.tolist() == [0, 0, 0, 0, 0, 0, 1] and g2.tolist() == [1, 1, 1, 1, 2, 2, 2]
    g2_, G2, _, _ = gridhip.average_groups(a1, a2, t, ntime=2, uvw=(uvw[:, 0], uvw[:, 1], uvw[:, 2]), bda=4)
    assert G2 == 4 + 2 + 2 and g2_.tolist() == (np.array([0, 4, 6])[bl] + t // np.array([2, 4, 4])[bl]).tolist()
    g, G, _, _ = gridhip.average_groups([], [], [])
    assert G == 1 and g.numel() == 0
    for kw in (dict(ntime=0), dict(nchan=0), dict(bda=8), dict(ntime=4, bda=2, uvw=uvw), dict(chan=ch[:-1]),
               dict(uvw=uvw[:-1], bda=8)):
        with pytest.raises(ValueError):
            gridhip.average_groups(a1, a2, t, **kw)
    with pytest.raises(ValueError):
        gridhip.average_groups(a1, a2[:-1], t)
