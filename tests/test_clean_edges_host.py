"""The preconditions of tests/clean_edge_cases.py, on the restatements alone: no GPU.

- Every exact fixture equals its np.longdouble rerun: no operation of the run rounded, so a kernel owes the same bits.
- Every tie fixture meets an exact tie (gap == 0), and a restatement whose peak() takes the HIGHEST flat index among
  equal maxima gives another component sequence: the fixture tells the two rules apart.
- Every fixture with components on the rim, or whose update region reaches it, gives another residual when the update region's clip is off by one.
- The three restatements (clean, msclean with scales = [0], mfclean with T = 1) give one another's bits."""
import numpy as np
import pytest

import clean_edge_cases as E

TIES = E.tie_fixtures()
RIM = E.rim_fixtures() + E.straddle_fixtures()
EXACT = TIES + RIM + E.misaligned_fixtures()
ids = lambda fs: [f.name for f in fs]  # noqa: E731


def assert_exact(f):
    model, res, stats = E.reference("clean", f)
    if f.mask is None:
        lm, lr, ls = E.reference("clean", f, np.longdouble)
        assert np.array_equal(lm, model) and np.array_equal(ls, stats), f.name
    else:
        lr, _ = E.mutant(f, dtype=np.longdouble)
    assert np.array_equal(lr, res), f"{f.name}: an operation rounded (lower niter)"
    assert stats[0] == f.niter, (f.name, stats)
    return model, res, stats


@pytest.mark.parametrize("f", EXACT, ids=ids(EXACT))
def test_exact_fixtures_equal_their_longdouble_rerun(f):
    model, res, stats = assert_exact(f)
    own, seq = E.mutant(f)
    assert np.array_equal(own, res) and len(seq) == f.niter, f"{f.name}: the unchanged mutant is not the restatement"
    if f.mask is None:
        for loop in ("ms0", "mf1"):
            m, r, s = E.reference(loop, f)
            assert E.same_bits(m, model) and E.same_bits(r, res) and s[0] == stats[0] and s[2] == stats[2], (f.name, loop)


@pytest.mark.parametrize("f", TIES, ids=ids(TIES))
def test_tie_fixtures_meet_a_tie_and_tell_the_rules_apart(f):
    trace = []
    E.reference("clean", f, trace=trace)
    gaps = [t[-1] for t in trace[:f.niter]]
    assert gaps[0] == 0.0, (f.name, gaps)
    taken = {t[0] for t in trace}
    if f.cells:
        assert {y * f.N + x for y, x, _ in f.cells} <= taken, f"{f.name}: a tied cell is never taken"
    assert E.mutant(f, highest=True)[1] != E.mutant(f)[1], f"{f.name}: the highest-index rule gives the same sequence"


def test_the_constant_image_starts_at_the_border_and_the_mask_moves_it():
    for N in (129, 130, 257):
        plain, masked = (next(f for f in TIES if f.name == f"h-constant-{w}-N{N}") for w in ("border", "masked"))
        assert E.mutant(plain)[1][0] == 3 * N + 3 and E.mutant(masked)[1][0] == 3 * N + 3 + 5


def test_the_sign_is_the_lower_cells():
    for f in TIES:
        if f.name.startswith("g-"):
            model = E.reference("clean", f)[0]
            y, x, v = f.cells[0]
            assert v < 0 and model[y, x] < 0 and E.mutant(f)[1][0] == y * f.N + x, f.name


def test_the_big_fixture():
    """N = 2049: exact, ten ties in twelve picks, told apart from the highest-index rule"""
    f = E.big_fixture()
    ntx = (f.N + E.TW - 1) // E.TW
    entries = [(y // E.TH) * ntx + x // E.TW for y, x, _ in f.cells]
    assert entries == [88, 1112, 700, 144, 2192] and ntx * ((f.N + E.TH - 1) // E.TH) == 2193
    trace = []
    model, res, stats = E.reference("clean", f, trace=trace)
    lr, seq = E.mutant(f, dtype=np.longdouble)
    assert np.array_equal(lr, res) and seq == [k for k, _ in trace] and stats[0] == 12
    assert sum(1 for _, g in trace if g == 0.0) == 10, trace
    assert E.mutant(f, highest=True)[1] != seq


# (a wide border keeps the components in the middle; of the straddle fixtures only the patch = 65 region 126 .. 256 of
# the peak at x = 191 reaches the last column)
ON_THE_RIM = [f for f in E.rim_fixtures() if f.border == 0]
REACHES_THE_RIM = ON_THE_RIM + [f for f in E.straddle_fixtures() if "patch65" in f.name]


@pytest.mark.parametrize("f", REACHES_THE_RIM, ids=ids(REACHES_THE_RIM))
def test_rim_fixtures_notice_a_clip_that_is_off_by_one(f):
    res, seq = E.mutant(f)
    if f in ON_THE_RIM:
        assert any(f.N - 1 in divmod(k, f.N) for k in seq), f"{f.name}: no component in the last row or column"
    assert not np.array_equal(E.mutant(f, clip=2)[0], res), f"{f.name}: the clip's last row and column go unnoticed"


def test_what_the_rim_product_holds():
    """10 N x 5 patches x 2 borders; clean_check refuses none (2 * ((N - 1) // 2) < N).  N = 1 and N = 2 have one border
    (10 fewer) and N = 1 one patch twice (1 fewer)."""
    names = [f.name for f in E.rim_fixtures()]
    assert len(names) == len(set(names)) == 10 * 5 * 2 - 2 * 5 - 1
    for f in E.rim_fixtures():
        assert 2 * f.border < f.N and f.patch >= 0


# ---- the wide forms ------------------------------------------------------------------------------------------------------------
WIDE = E.wide_tie_fixtures() + E.wide_rim_fixtures() + E.wide_misaligned_fixtures()


def assert_wide_trace(w):
    """the gap is exactly 0 at the picks meant to tie and above 1e-8 at every other pick; every stamp is taken"""
    model, res, stats, trace = E.wide_reference(w)
    gaps = [t[-1] for t in trace]
    assert stats[0] == w.niter == len(gaps), (w.name, stats)
    for i, g in enumerate(gaps):
        assert (g == 0.0) if i in w.ties else (g > 1e-8), f"{w.name}: pick {i} has gap {g}; all {gaps}"
    if w.stamp:
        assert {y * w.N + x for y, x, _ in w.cells} <= {t[-2] for t in trace}, f"{w.name}: a stamp is never taken"
        assert trace[0][-2] == min(y * w.N + x for y, x, _ in w.cells)
    return trace


@pytest.mark.parametrize("w", WIDE, ids=ids(WIDE))
def test_wide_fixtures_tie_where_they_are_meant_to_and_nowhere_else(w):
    assert_wide_trace(w)


def test_the_big_wide_fixtures():
    """N = 2049.  The restatements take about 5 s (msclean, two scales, 3 picks: most of it is the set-up convolutions)
    and 3 s (mfclean, T = 2, 5 picks) here."""
    for w in E.wide_big_fixtures():
        trace = assert_wide_trace(w)
        ks = [t[-2] for t in trace]
        cells = sorted(y * w.N + x for y, x, _ in w.cells)
        assert ks[:3] == cells, (w.name, ks)  # entry 88, then 700 before 1112


SCALE_TIES = E.scale_tie_fixtures()


@pytest.mark.parametrize("f", SCALE_TIES, ids=ids(SCALE_TIES))
def test_the_tie_between_scales(f):
    """b_s (p_s / q_s) is the same double for s = 0 and s = 1 at every pick, the restatement takes s = 0 every time, and
    the run is the delta-only run bit for bit (so it is exact as that one is)."""
    import msclean_ref
    psf = np.array(E.exact_psf(f.N))
    m, P, q = msclean_ref.setup(psf, list(E.SCALE_TIE["scales"]))
    assert q[0] == q[1] == 1.0 and m[1].shape == (1, 1) and m[1][0, 0] == 1.0 and np.array_equal(P[(1, 1)], psf)
    trace = []
    model, res, stats = E.scale_tie_reference(f, trace)
    assert len(trace) == f.niter and all(s == 0 and g == 0.0 for s, _, g in trace), trace
    assert stats[3] == 0 and stats[6] == f.niter and stats[7] == 0
    m0, r0, _ = E.reference("ms0", f)
    assert E.same_bits(model, m0) and E.same_bits(res, r0)


def test_there_are_four_scale_tie_fixtures():
    assert len(SCALE_TIES) == 4
