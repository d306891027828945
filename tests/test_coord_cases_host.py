"""The streams of tests/coord_cases.py have the structure they are named for (no GPU): every class of candidate is
populated at every grid and Q the GPU module runs, the two oracles and weights_ref agree on every candidate, the
integer data is exact in fp64, and a mirrored stream is not the mirror of its cells.

Class floors are per grid (H, Wd) and Q, counted over the candidates of the grid's two axes.  A 64 x 64 grid has no
contraction-sensitive candidate at all (p * 64 is exact): that is why a test at N = 64 alone cannot notice a fused
multiply-add in the coordinate rule.

The high clamp (round gives Q) is unreachable: among five doubles either side of every target, at every Q and at the
sizes 33 .. 4096 listed in HIGH_SIZES, no candidate reaches it, so the streams hold none and only the low clamp is
exercised on the device."""
import numpy as np
import pytest

import coord_cases as cc
import sorted_cases as sc
import weights_ref
from oracle import gridref_np as P

GRID_Q = [(H, Wd, Q) for H, Wd in cc.GRIDS for Q in cc.QS]
HIGH_SIZES = cc.AXES + (128, 255, 256, 511, 1000, 1023, 2048, 4095, 4096)


def class_sizes(H, Wd, Q):
    tot = np.zeros(6, dtype=np.int64)
    for n in (H, Wd):
        tot += [int(m.sum()) for m in cc.classify(n, Q, cc.candidates(n, Q))]
    return cc.Classes(*tot)


@pytest.mark.parametrize("H,Wd,Q", GRID_Q)
def test_class_floors(H, Wd, Q):
    c = class_sizes(H, Wd, Q)
    print(H, Wd, Q, c)
    assert c.cell_tie >= 100 and c.sub_tie >= 100 and c.low_clamp >= 15
    if Q in (2, 4, 5, 8):
        assert c.rint >= 100
    if (H, Wd) == (64, 64):
        assert c.contraction == 0
    else:
        assert c.contraction >= 30
    assert c.high_clamp == 0        # (module docstring)


@pytest.mark.parametrize("Q", cc.QS)
def test_high_clamp_is_unreachable(Q):
    for n in HIGH_SIZES:
        p = cc.candidates(n, Q, 5)
        _, r, _, _ = cc.rule_from_x(np.float64(n // 2) + p * np.float64(n), Q)
        assert r.max() <= Q - 1 and r.min() >= -1, n


@pytest.mark.parametrize("n", cc.AXES)
def test_every_low_clamp_is_a_cell_tie_and_every_class_is_a_tie(n):
    for Q in cc.QS:
        c = cc.classify(n, Q, cc.candidates(n, Q))
        assert not (c.low_clamp & ~c.cell_tie).any()
        assert not (c.rint & ~c.sub_tie).any()


@pytest.mark.parametrize("n", cc.AXES)
def test_oracles_agree_on_every_candidate(oracle, n):
    for Q in cc.QS:
        p = cc.candidates(n, Q)
        cell, sub = cc.rule(n, Q, p)
        for got in (P.frac_coord(n, Q, p), oracle.frac_coord(n, Q, p)):
            assert np.array_equal(got[0], cell) and np.array_equal(got[1], sub), Q


@pytest.mark.parametrize("N", cc.AXES)
def test_weights_ref_cells_agree_at_q1(N):
    """theta = 0.25, lam = 4 N, as test_gpu_image_ops has it; the classes are counted on u / lam, which is what every
    implementation bins"""
    lam = 4 * N
    u = cc.wavelengths(cc.candidates(N, 1), lam)
    p = u / np.float64(lam)
    c = cc.classify(N, 1, p)
    assert c.cell_tie.sum() >= 100 and c.low_clamp.sum() >= 15 and (N == 64 or c.contraction.sum() >= 15)
    v = np.random.default_rng(N).permutation(u)
    x, _ = cc.rule(N, 1, p)
    y, _ = cc.rule(N, 1, v / np.float64(lam))
    want = np.where((x >= 0) & (x < N) & (y >= 0) & (y < N), y * N + x, -1)
    assert np.array_equal(weights_ref.cells(N, lam, u, v), want)
    assert (want < 0).sum() >= 10 and (want >= 0).sum() >= 100


@pytest.mark.parametrize("H,Wd,Q", GRID_Q)
def test_integer_data_is_exact(H, Wd, Q):
    s = cc.tie_stream(H, Wd, Q)
    assert len(s.u) == len(s.v) == len(s.wb) == len(s.vis) and 100 < len(s.u) < 20000
    assert s.nbad >= 2 and (~s.keep).sum() == s.nbad
    for gh, gw in cc.SUPPORTS:
        g = cc.int_gcf(Q, gh, gw)
        assert g.shape == (cc.W, Q, Q, gh, gw)
        for a in (g.real, g.imag, s.vis.real, s.vis.imag):
            assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= cc.VMAX
        assert cc.sum_bound(len(s.u), gh, gw) < 2 ** 53
        # neighbouring slices differ along each axis (the last sub-cell's neighbour is the next cell's first)
        f = g.reshape(cc.W, Q, Q, -1)
        assert (f[0] != f[1]).any(axis=-1).all()
        if Q > 1:
            assert (f != np.roll(f, 1, axis=1)).any(axis=-1).all() and (f != np.roll(f, 1, axis=2)).any(axis=-1).all()
    G = cc.int_grid(H, Wd)
    assert np.array_equal(G.real, np.rint(G.real)) and np.abs(G.real).max() <= cc.VMAX


@pytest.mark.parametrize("H,Wd,Q", cc.HARD)
def test_oracle_sums_are_the_integer_sums(oracle, H, Wd, Q):
    """the C oracle on the integer stream equals an int64 evaluation, and the largest partial sum is far below 2^53"""
    s = cc.tie_stream(H, Wd, Q)
    gh, gw = 5, 5
    g = cc.int_gcf(Q, gh, gw)
    k = s.keep
    re, im, bound = sc.int_eval(g, H, Wd, s.u[k], s.v[k], s.wb[k], vis=s.vis[k])
    assert bound < 2 ** 53 and bound <= cc.sum_bound(len(s.u), gh, gw)
    ref = oracle.convgrid2(g, np.zeros((H, Wd), dtype=np.complex128), s.u[k], s.v[k], s.wb[k], s.vis[k])
    assert np.array_equal(ref.real, re) and np.array_equal(ref.imag, im) and ref.any()
    G = cc.int_grid(H, Wd)
    re, im, bound = sc.int_eval(g, H, Wd, s.u[k], s.v[k], s.wb[k], G=G)
    d = oracle.degrid2(g, G, s.u[k], s.v[k], s.wb[k])
    assert bound < 2 ** 53 and np.array_equal(d.real, re) and np.array_equal(d.imag, im) and d.any()


@pytest.mark.parametrize("n", cc.AXES)
def test_mirrored_candidates_do_not_land_in_the_mirrored_cell(n):
    """floor(.5 + x) is no odd function: the imagers bin p and -p separately, and on these streams they have to"""
    for Q in cc.QS:
        p = cc.candidates(n, Q)
        cell, _ = cc.rule(n, Q, p)
        mcell, _ = cc.rule(n, Q, -p)
        assert (mcell != 2 * (n // 2) - cell).sum() >= 50, Q


@pytest.mark.parametrize("n", cc.AXES)
def test_ulp_pairs_straddle_a_step(n):
    for Q in cc.QS:
        a, b = cc.ulp_pairs(n, Q)
        assert len(a) >= 20 and np.array_equal(np.nextafter(a, np.inf), b)
        ca, fa = P.frac_coord(n, Q, a)
        cb, fb = P.frac_coord(n, Q, b)
        assert ((ca != cb) | (fa != fb)).all()
        assert ((ca == cb) & (fa != fb)).sum() >= (10 if Q > 1 else 0)      # the sub-cell alone changes


@pytest.mark.parametrize("H,n", [(49, 33), (49, 49), (64, 64), (100, 257), (100, 100)])
def test_grid_rule_candidates(H, n):
    """H * p = j - 0.5 exactly for many j, cells either side of each, and the one p where 0.5 + H * p rounds up"""
    p = cc.grid_candidates(H, n)
    hp = np.float64(H) * p
    assert (hp - np.floor(hp) == 0.5).sum() >= n // 2
    c = cc.grid_rule(H, p)
    assert len(np.unique(c)) >= n + 4
    odd = p[np.abs(hp - 0.49999999999999994) < 1e-16]
    assert len(odd) and (cc.grid_rule(H, odd) == 1).any()
    G = np.zeros((H, n), dtype=np.complex128)
    P.grid(G, p, p[::-1], np.ones(len(p)))
    x = H // 2 + c.astype(np.int64)
    y = x[::-1]
    assert G.real.sum() == ((x >= 0) & (x < n) & (y >= 0) & (y < H)).sum()


@pytest.mark.parametrize("n,S", [(33, 1), (49, 17), (64, 7), (257, 5)])
def test_extremes(n, S):
    e = cc.extremes(n, S)
    assert np.isnan(e).sum() == 1 and np.isinf(e).sum() == 2 and (e == 0).sum() == 2 and (np.abs(e) == 5e-324).sum() == 2
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.float64(n // 2) + e * np.float64(n)
        cell = np.floor(x + 0.5)
    t = cc.touches(n, S, cell)
    fin = np.isfinite(cell) & (np.abs(cell) < 2.0 ** 62)
    assert t.sum() >= 6 and (~t & fin).sum() >= 4            # both sides of the last footprint that touches, each end
    assert (np.abs(cell[fin]) >= 2.0 ** 31 - n).sum() == 6 and (cell[fin] >= 2.0 ** 31).sum() == 3 and (~fin).sum() == 11
