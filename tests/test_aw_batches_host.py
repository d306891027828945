"""The preconditions of tests/aw_batch_cases.py, with the oracle and numpy alone: no GPU.

- Every cut fixture has, in its arrays, the property it is named for: the batch sizes, the run of equal keys across a
  cut, the batch of dropped visibilities only, the batch whose one antenna pair is older than the batch.
- The figures test_gpu_aw_batches.py demands of kernels_built, last_dropped() and aw_tables_built come from here; in at
  least one fixture the per-batch sum of distinct keys exceeds the stream's distinct count, so a kernels_built that
  ignored the batches would not pass.
- The wrap fixtures: the coordinates give the slices they were placed for under oracle.frac_coord, and in whatever order
  the keys are inserted, at least three of the chosen ones end in slots 0.. of the 1024-slot table, in every batch.

The whole file takes 0.6 s here (one CPU core; the key sets are Python sets of a few hundred tuples)."""
import numpy as np
import pytest

import aw_batch_cases as E

CUTS = {c.name: c for c in E.cut_cases()}


@pytest.mark.parametrize("c", E.all_cases(), ids=lambda c: c.name)
def test_shapes_are_the_small_ones(c):
    n = len(c.u)
    assert 64 <= c.N <= 96 and c.S in (5, 9, 12) and n <= 600 and (c.S < 12 or n <= 300)
    for a in (c.v, c.wb, c.a1, c.a2, c.vis):
        assert len(a) == n
    assert np.nanmax(np.abs(c.u)) <= 0.4 + 1e-3 and np.nanmax(np.abs(c.v)) <= 0.4 + 1e-3  # nothing dropped at the rim
    assert E.batches(c)[0] == (0, min(c.B, n)) and E.batches(c)[-1][1] == n
    if c.name in CUTS:
        assert 2 <= c.W <= 3 and c.Q == 2 and 4 <= c.A <= 5


def test_batch_sizes():
    c = CUTS["multiple"]
    assert len(c.u) % c.B == 0 and len(c.u) // c.B >= 3
    c = CUTS["plus-one"]
    assert len(c.u) % c.B == 1 and E.batches(c)[-1] == (len(c.u) - 1, len(c.u))
    c = CUTS["one-each"]
    assert c.B == 1 and len(E.batches(c)) == len(c.u) > 1


def test_a_run_of_equal_keys_straddles_a_cut(oracle):
    c = CUTS["straddle"]
    k = E.keys(c, oracle.frac_coord)
    cut = c.B
    assert E.kept(c)[cut - 1] and E.kept(c)[cut]
    assert np.array_equal(k[cut - 1], k[cut]) and (c.u[cut - 1], c.v[cut - 1]) == (c.u[cut], c.v[cut])
    # ... and the run is longer than the two of them, on both sides
    assert np.array_equal(k[cut - 2], k[cut]) and np.array_equal(k[cut + 1], k[cut])


def test_one_batch_holds_dropped_visibilities_only():
    c = CUTS["dropped-batch"]
    keep = E.kept(c)
    per = [int(keep[lo:hi].sum()) for lo, hi in E.batches(c)]
    assert per.count(0) == 1 and 0 < per.index(0) < len(per) - 1  # a batch in the middle
    lo, hi = E.batches(c)[per.index(0)]
    ways = [(c.wb[lo:hi] >= c.W).any(), (c.wb[lo:hi] < 0).any(), (c.a1[lo:hi] == -1).any(), (c.a2[lo:hi] == c.A).any(),
            np.isnan(c.u[lo:hi]).any(), np.isnan(c.v[lo:hi]).any()]
    assert all(ways)
    # the other batches keep most of theirs, and drop their first or last one
    assert all(p >= c.B - 2 for p in per if p) and not keep[0] and not keep[len(c.u) - 1]


def test_one_batch_has_only_a_pair_that_an_earlier_batch_met_first():
    c = CUTS["old-pair"]
    assert E.kept(c).all()
    pairs = [set(zip(c.a1[lo:hi].tolist(), c.a2[lo:hi].tolist())) for lo, hi in E.batches(c)]
    assert len(pairs) == 3 and pairs[1] == {(2, 1)} and (2, 1) in pairs[0] and len(pairs[0]) > 1
    assert (2, 1) not in pairs[2] and len(pairs[2]) > 1
    first = next(k for k in range(len(c.u)) if (c.a1[k], c.a2[k]) == (2, 1))
    assert first < c.B


def test_figures_and_that_batches_matter(oracle):
    more = []
    for c in E.all_cases():
        per, total, dropped, whole = E.figures(c, oracle.frac_coord)
        assert len(per) == -(-len(c.u) // c.B) and total == sum(per) and total >= whole
        nan = np.isnan(c.u) | np.isnan(c.v)
        index = ~((c.wb >= 0) & (c.wb < c.W) & (c.a1 >= 0) & (c.a1 < c.A) & (c.a2 >= 0) & (c.a2 < c.A))
        assert not (nan & index).any() and np.array_equal(nan | index, ~E.kept(c))  # one cause each
        assert dropped == int(index.sum()) and all(p <= c.B for p in per)
        if total > whole:
            more.append(c.name)
    # a kernels_built that ignored the batches would report `whole`
    assert "straddle" in more and "wrap-two" in more, more
    per, total, dropped, whole = E.figures(CUTS["dropped-batch"], oracle.frac_coord)
    # 48 + 6 dropped, a third of them by a NaN coordinate: off the grid, which gridhip_last_dropped does not count
    c = CUTS["dropped-batch"]
    assert per.count(0) == 1 and int((~E.kept(c)).sum()) == 48 + 6 and dropped == 32 + 4
    per, total, dropped, whole = E.figures(CUTS["one-each"], oracle.frac_coord)
    assert per == [1] * 60 and whole < 60  # keys repeat over a baseline's dumps
    # repetition inside a batch, too: the cache has something to do
    per, total, dropped, whole = E.figures(CUTS["multiple"], oracle.frac_coord)
    assert total < int(E.kept(CUTS["multiple"]).sum())


def test_the_hash_is_restated_as_the_kernel_states_it():
    # (key * 0x9E3779B97F4A7C15 mod 2^64) >> 32 & 1023, on numbers worked by hand: 0 -> 0; 1 -> 0x9E3779B9 & 1023
    assert E.home(0) == 0 and E.home(1) == 0x9E3779B9 & 1023 == 0x1B9
    assert E.home(2) == ((2 * 0x9E3779B97F4A7C15) >> 32) & 1023


@pytest.mark.parametrize("c", E.wrap_cases(), ids=lambda c: c.name)
def test_wrap_fixture(oracle, c):
    n = len(c.u)
    assert c.A == 2 and (c.a1 == 0).all() and (c.a2 == 1).all()  # one pair: slot 0, the key is the slice
    assert c.W * c.Q * c.Q == 4096 and c.B <= 512 and all(2 * (hi - lo) <= E.HSLOTS for lo, hi in E.batches(c))
    # the coordinates give the slices they were placed for
    sl = E.slices_of(c, oracle.frac_coord)
    x, xf = oracle.frac_coord(c.N, c.Q, c.u)
    y, yf = oracle.frac_coord(c.N, c.Q, c.v)
    assert np.array_equal(xf, (c.u * c.N) * c.Q % c.Q) and np.array_equal(yf, (c.v * c.N) * c.Q % c.Q)
    assert (x >= 8).all() and (x < c.N - 8).all() and (y >= 8).all() and (y < c.N - 8).all()
    chosen = E.wrap_keys()[:10]
    assert len(chosen) >= 6 and all(E.home(k) in E.TAIL for k in chosen)
    rng = np.random.default_rng(1)
    for lo, hi in E.batches(c):
        ks = [int(k) for k in sl[lo:hi]]
        assert set(chosen) <= set(ks), "every batch meets every chosen key"
        if len(E.batches(c)) == 1:
            assert len(set(ks)) >= 0.45 * E.HSLOTS  # near the 50 % the table is sized for
        orders = [ks, ks[::-1], sorted(ks), sorted(ks, reverse=True)] + [list(rng.permutation(ks)) for _ in range(20)]
        for order in orders:
            where = E.probe(order)
            wrapped = [k for k in chosen if where[k] < E.TAIL[0]]
            # (three slots for the chosen keys' homes: whoever comes after the third goes round)
            assert len(wrapped) >= 3 and len(wrapped) >= len(chosen) - 3, (c.name, len(wrapped))
            assert all(where[k] < 64 for k in wrapped)  # round to the table's first slots, not lost somewhere
    if len(E.batches(c)) == 2:
        (l0, h0), (l1, h1) = E.batches(c)
        assert set(sl[l0:h0].tolist()) & set(sl[l1:h1].tolist()) == set(chosen)  # the wrapped keys recur, nothing else
