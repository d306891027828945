"""Preconditions of test_gpu_sorted_matrix.py, on the CPU: every stream of sorted_cases.py has the structure it is named
for (by the reference's coordinate rule, oracle/gridref_np.frac_coords), the two densities of the matrix really give
long and short runs, and the integer streams are exact: the C oracle's fp64 result equals an evaluation in int64, and
no partial sum can leave the integers fp64 holds exactly."""
import numpy as np
import pytest

import sorted_cases as K


def test_shape_classes_are_what_the_issue_table_says():
    """the representatives of part C cover every compile-time class, and all 28 supports fall into one of them"""
    c = {(S, d): K.shape_class(S, d) for S in K.SUPPORTS for d in (False, True)}
    assert c[5, False]["steps"] == 1 and c[5, False]["tail"] == 25                     # one partial step
    assert c[8, False]["steps"] == 1 and c[8, False]["tail"] == 64                     # one full step
    assert c[15, False]["extra"] == 1 and c[15, False]["pair"] and c[15, False]["steps"] == 4
    assert c[16, False]["steps"] == 4 and c[16, False]["tail"] == 64 and c[16, False]["parts"] == 1
    assert c[17, False]["extra"] == 1 and c[17, False]["pair"] and c[17, False]["steps"] == 5 and c[17, False]["parts"] == 1
    assert c[17, True]["parts"] == 2 and c[17, True]["extra"] == 0
    assert c[18, False]["parts"] == 2 and c[18, False]["steps"] == 6
    assert c[23, False]["rem"] != 0 and c[17, True]["rem"] != 0                        # parts of unequal length
    assert c[31, False]["extra"] == 1 and c[31, False]["steps"] == 15 and c[31, False]["parts"] == 3
    assert c[31, True]["parts"] == 4 and c[31, True]["steps"] == 16
    assert c[32, False]["steps"] == 16 and c[32, False]["tail"] == 64
    # the only supports with extra taps or the pair path are among the representatives
    assert {S for S in K.SUPPORTS if c[S, False]["extra"]} == {15, 17, 31}
    assert {S for S in K.SUPPORTS if c[S, False]["pair"]} == {15, 17}
    assert {c[S, d]["parts"] for S in K.SUPPORTS for d in (False, True)} == {1, 2, 3, 4}
    for key in ("parts", "pair", "extra"):
        for d in (False, True):
            assert {c[S, d][key] for S in K.CLASS_SUPPORTS} == {c[S, d][key] for S in K.SUPPORTS}, key
    assert not any(c[S, True]["extra"] or c[S, True]["pair"] for S in K.SUPPORTS)


@pytest.mark.parametrize("S", K.SUPPORTS)
def test_the_two_densities_give_long_and_short_runs(S):
    """B1 / B2: records per (tile, slice) with the default small-grid tile (16 x 16) and with the production tile.
    "long" must mean many visibilities per run even in the small tile, "short" about one - and still runs of several
    in the production tile, which holds twenty times the cells."""
    mean = {}
    for name, (W, Q) in K.DENSITIES.items():
        _, u, v, wb, _ = K.uniform_case(S, K.H1, K.WD1, W, Q, S, K.N1, K.SPREAD1)
        mean[name] = (K.mean_run_length(K.H1, K.WD1, W, Q, S, (K.SMALL_TILE,) * 2, u, v, wb),
                      K.mean_run_length(K.H1, K.WD1, W, Q, S, K.PROD_TILE[S], u, v, wb))
    print(S, mean)
    assert mean["long"][0] > 10 and mean["long"][1] > 100     # runs of many visibilities; of more than a block
    assert 1.0 <= mean["short"][0] < 1.5 and 2 < mean["short"][1] < 12
    # footprints over all four edges
    _, u, v, _, _ = K.uniform_case(S, K.H1, K.WD1, 2, 2, S, K.N1, K.SPREAD1)
    _, x, y, _ = K.slices_of(K.H1, K.WD1, 2, u, v, np.zeros(K.N1, dtype=np.int64))
    h = S // 2
    for lo, hi, n in ((x - h, x - h + S, K.WD1), (y - h, y - h + S, K.H1)):
        assert ((lo < 0) & (hi > 0)).any() and ((lo < n) & (hi > n)).any()


def test_production_tile_table():
    assert K.PROD_TILE[15] == (65, 89) and set(K.PROD_TILE) == set(K.SUPPORTS)
    for S, (tx, ty) in K.PROD_TILE.items():
        rows, cols = ty + S - 1, tx + S - 1
        pitch = cols + (S - cols) % 32
        assert rows * pitch * 8 <= 65528 and (rows + 1) * pitch * 8 > 65528 or ty == 128, S   # the tallest that fits


@pytest.mark.parametrize("S", K.SUPPORTS)
def test_bigtile_windows(S):
    """B3: a window at the corner (origins outside the grid, taps clipped) and one at the centre, long runs"""
    _, u, v, wb, _, side = K.window_case(S, S)
    _, x, y, sl = K.slices_of(K.N3, K.N3, K.Q3, u, v, wb)
    h = K.N1 // 2
    assert x[:h].min() < 0 and y[:h].min() < 0 and x[:h].min() - S // 2 + S > 0       # every one keeps a tap inside
    assert max(x[:h].max(), y[:h].max()) <= side
    assert np.abs(x[h:] - K.N3 // 2).max() <= side / 2 + 1 and np.abs(y[h:] - K.N3 // 2).max() <= side / 2 + 1
    assert K.mean_run_length(K.N3, K.N3, K.W3, K.Q3, S, (97, 106), u, v, wb) > 50   # (no tile is larger than 97 x 106)


def sorted_run_lengths(s):
    ok, _, _, sl = K.slices_of(K.HC, K.WDC, s.Q, s.u, s.v, s.wb)
    ok &= s.wb < s.W
    return ok, np.sort(sl[ok], kind="stable")


def test_streams_have_the_structure_they_are_named_for():
    for n in K.ONE_RUN_LENGTHS:
        s = K.one_run(n)
        ok, sl = sorted_run_lengths(s)
        assert ok.all() and len(sl) == n and len(set(sl)) == 1
    # odd and even lengths (the pair path), block boundaries (64) crossed, a partial last block
    assert {n % 2 for n in K.ONE_RUN_LENGTHS} == {0, 1} and {63, 64, 65, 129} <= set(K.ONE_RUN_LENGTHS)

    s = K.singles()
    ok, sl = sorted_run_lengths(s)
    assert (~ok).sum() == 3 == s.ndrop and np.array_equal(sl, np.arange(256))            # every slice exactly once
    assert np.isnan(s.u).sum() == 1 and np.isnan(s.v).sum() == 1 and (s.wb == s.W).sum() == 1

    starts = set()
    for rev in (False, True):
        s = K.ladder(rev)
        ok, sl = sorted_run_lengths(s)
        lens = K.run_lengths(sl)
        want = np.arange(1, K.LADDER + 1)
        assert (~ok).sum() == 3 and len(sl) == 300 and np.array_equal(lens, want[::-1] if rev else want)
        first = np.concatenate([[0], np.cumsum(lens)[:-1]])
        starts |= set(first % 64)
        # a run straddles each 64-record boundary of the list
        for b in (64, 128, 192, 256):
            assert ((first < b) & (first + lens > b)).any(), (rev, b)
        if rev:   # ... and one covers lanes 60..67 of the first two blocks
            assert ((first <= 60) & (first + lens > 67)).any()
    assert len(starts) >= 40   # run starts on 40 or more of the 64 lane positions (two orders of 24 runs each)

    for k in range(4):
        s = K.few(k)
        _, x, y, _ = K.slices_of(K.HC, K.WDC, s.Q, s.u, s.v, s.wb)
        cells, counts = np.unique(np.stack([x, y]), axis=1, return_counts=True)
        assert sorted(counts) == [1 + k, 5 + k, 9 + k, 13 + k] and cells.shape[1] == 4
    assert sorted(c for k in range(4) for c in (1 + k, 5 + k, 9 + k, 13 + k)) == list(range(1, 17))
    for S in K.CLASS_SUPPORTS:   # four tiles under the small tile and under the production tile of every support used
        for tx, ty in ((K.SMALL_TILE,) * 2, K.PROD_TILE[S]):
            assert len({((cx - S // 2) // tx, (cy - S // 2) // ty) for cx, cy in K.FEW_CELLS}) == 4
        for cx, cy in K.FEW_CELLS:   # footprints inside the grid
            assert cx - S // 2 >= 0 and cy - S // 2 >= 0 and cx - S // 2 + S <= K.WDC and cy - S // 2 + S <= K.HC

    for n in K.BATCH_LENGTHS:
        s = K.batches(n)
        ok, sl = sorted_run_lengths(s)
        assert ok.all() and len(sl) == n and s.opts == {"chunk": 64} and len(set(sl)) == 8

    for S in (15, 31):
        for tile in ((K.SMALL_TILE,) * 2, K.PROD_TILE[S]):
            s = K.window(tile, S)
            _, x, y, sl = K.slices_of(K.HC, K.WDC, s.Q, s.u, s.v, s.wb)
            assert len(set(sl)) == 1 and len(x) == (tile[0] + 2) * (tile[1] + 2)
            assert len(set(zip(x, y))) == len(x)                                        # every cell once
            # every position of a footprint origin in a tile, whatever the tile's origin
            pos = {((cx - S // 2) % tile[0], (cy - S // 2) % tile[1]) for cx, cy in zip(x, y)}
            assert len(pos) == tile[0] * tile[1]
    assert len(K.window(K.PROD_TILE[15], 15).u) == 6097

    for W, ng in K.WGROUP_CASES:
        s = K.wgroups(W, ng)
        ok, sl = sorted_run_lengths(s)
        g = min(ng, W)
        assert ok.all() and len(sl) == 2000 and len(set(sl)) == W * 4 and (W % g != 0 or g != ng)
        # the planes of a group start at ceil(grp * W / g): check against the group each plane is binned into
        grp = np.arange(W) * g // W
        for k in range(g):
            assert np.flatnonzero(grp == k).min() == -(-k * W // g)
        if W == 5:   # rounding down would name another plane for groups 1 and 2
            assert [k * W // g for k in range(g)] != [-(-k * W // g) for k in range(g)]


def test_every_stream_sits_where_it_should():
    """all records of streams 1, 2, 3, 5 and 7 at one cell: one tile and one footprint origin under any geometry"""
    for s in K.structured_streams():
        if s.name.startswith("few"):
            continue
        ok, x, y, _ = K.slices_of(K.HC, K.WDC, s.Q, s.u, s.v, s.wb)
        assert set(zip(x[ok], y[ok])) == {K.CELL}, s.name


@pytest.mark.parametrize("S", K.CLASS_SUPPORTS)
def test_integer_streams_are_exact_in_fp64(oracle, S):
    """The oracle's fp64 result equals the evaluation in int64, and the sum of |products| per output element - an upper
    bound of every partial sum in any order of the atomics - stays far below 2^53: the GPU comparison may be
    np.array_equal.  The bound: |product component| <= 2 * 3 * 3 = 18, at most max(n, S^2) <= 6097 of them per element,
    so below 2^17."""
    streams = K.structured_streams()
    if S in (15, 31):
        streams += [K.window((K.SMALL_TILE,) * 2, S), K.window(K.PROD_TILE[S], S)]
    worst = 0
    for s in streams:
        n = len(s.u)
        gcf, vis, G = K.int_tables(S, s.W, s.Q, n)
        keep = np.isfinite(s.u) & np.isfinite(s.v) & (s.wb < s.W)
        u, v, wb = s.u[keep], s.v[keep], s.wb[keep]
        ref = oracle.convgrid2(gcf, np.zeros((K.HC, K.WDC), dtype=np.complex128), u, v, wb, vis[keep])
        re, im, m1 = K.int_eval(gcf, K.HC, K.WDC, s.u, s.v, s.wb, vis=vis)
        assert np.array_equal(ref.real, re) and np.array_equal(ref.imag, im), s.name
        dref = np.zeros(n, dtype=np.complex128)
        dref[keep] = oracle.degrid2(gcf, G, u, v, wb)
        re, im, m2 = K.int_eval(gcf, K.HC, K.WDC, s.u, s.v, s.wb, G=G)
        assert np.array_equal(dref.real, re) and np.array_equal(dref.imag, im), s.name
        assert not re[~keep].any() and not im[~keep].any()
        assert np.abs(ref).max() > 0 and np.abs(dref).max() > 0
        worst = max(worst, m1, m2)
    assert worst < 2 ** 17 < 2 ** 53


def test_aw_residue_stream():
    wk, ak, u, v, wb, a1, a2, vis, G = K.aw_residues()
    n, Q = K.AW8["n"], K.AW8["Q"]
    _, x, y, sl = K.slices_of(K.H4, K.WD4, Q, u, v, wb)
    assert len(u) == n and len(set(zip(x, y))) == 1                      # one cell: one tile, one batch (n < 2^20)
    keys = set(zip(a1, a2, sl))                                          # (a1, a2, wbin, yf, xf)
    D = len(keys)
    assert D >= 2 * K.AW_KEYS
    # kernels numbered 0 .. D - 1 in any order: residue r holds the indices r, r + 4096, ...
    held = np.bincount(np.arange(D) % K.AW_KEYS, minlength=K.AW_KEYS)
    assert (held >= 2).sum() >= 1000 and (held >= 2).all()
    assert K.AW8["A"] ** 2 * K.AW8["W"] * Q * Q >= 2 * K.AW_KEYS > 9 * 9 * 5 * 4 * 4
