"""Deblending in the source finder (option "sources_deblend"), the checks that need no GPU: the header carries the rule
and the option, the Python methods take `deblend`, and the restatement the GPU tests compare with (tests/deblend_ref.py)
splits a blended pair of Gaussians into two rows near the true positions whose sums add up to the island's."""
import inspect
import os

import numpy as np

import deblend_ref
import sources_ref
from conftest import ROOT

THETA = 0.1
PAIR = [(10.0, 11.6, 14.3), (6.0, 18.4, 16.2)]  # amplitude, x, y; sigma 2 cells


def pair_image(N=33, sigma=2.0):
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    img = np.zeros((N, N))
    for a, x, y in PAIR:
        img += a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2.0 * sigma * sigma))
    return img


KW = dict(thr=(1.0, 0.05), nsigma=(0.0, 0.0), correct=False)


def test_the_header_holds_the_rule_and_the_option():
    text = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    section = text[text.index("---- source finding"):text.index("---- phase shift and averaging")]
    assert "DEBLENDING" in section and '"sources_deblend"' in section
    options = text[:text.index("---- source finding")]
    assert '"sources_deblend"' in options
    for word in ("up[k]", "faint summit", "Chebyshev", "bit 3", "watershed"):
        assert word in section, word


def test_the_python_methods_take_deblend():
    import gridhip
    for cls in (gridhip.Context, gridhip.Imager):
        p = inspect.signature(cls.find_sources).parameters["deblend"]
        assert p.default == 0 and "deblend" in cls.find_sources.__doc__
    assert gridhip.SOURCE_BLENDED == deblend_ref.BLENDED == 8


def test_a_blended_pair_becomes_two_rows_that_add_up():
    img = pair_image()
    N = img.shape[0]
    one = sources_ref.find_sources(img, THETA, **KW)
    assert one["count"] == 1 and one["info"][0, 15] == 0
    for r in (1, 2, 4):
        two = deblend_ref.find_sources(img, THETA, r, **KW)
        assert two["count"] == 2 and two["stats"][3] == 2 and two["stats"][4] == 2
        info, comps = two["info"], two["comps"]
        assert np.all(info[:, 0] == one["info"][0, 0]) and np.all(info[:, 15].astype(int) & deblend_ref.BLENDED)
        assert info[0, 2] * N + info[0, 3] < info[1, 2] * N + info[1, 3]  # ascending peak cells
        assert info[:, 1].sum() == one["info"][0, 1]  # the basins partition the island
        for row, (a, x, y) in enumerate(PAIR):  # (the brighter one lies first in index order too)
            cx, cy = comps[row, 0] * N / THETA + N // 2, comps[row, 1] * N / THETA + N // 2
            print(f"r = {r}: ({cx:.3f}, {cy:.3f}) for ({x}, {y}), S = {info[row, 5]:.2f} for {2 * np.pi * 4.0 * a:.2f}")
            assert abs(cx - x) <= 0.2 and abs(cy - y) <= 0.2
            assert (info[row, 2], info[row, 3]) == (round(y), round(x))
        # S adds up: two orders of summation of the island's ncells terms, all positive
        n, mag = one["info"][0, 1], one["mags"][0, 0]
        assert abs(info[:, 5].sum() - one["info"][0, 5]) <= 4.0 * n * 2.0 ** -53 * mag


def test_one_peak_is_the_undeblended_row_and_deblend_0_is_sources_ref():
    img = pair_image()
    img[:, 16:] = 0.0  # the brighter one alone, cut
    a = sources_ref.find_sources(img, THETA, **KW)
    assert a["count"] == 1
    for r in (1, 3):
        b = deblend_ref.find_sources(img, THETA, r, **KW)
        assert b["count"] == 1 and np.array_equal(a["comps"], b["comps"]) and np.array_equal(a["info"], b["info"])
    c = deblend_ref.find_sources(img, THETA, 0, **KW)
    assert np.array_equal(a["comps"], c["comps"]) and np.array_equal(a["stats"], c["stats"])


def test_the_rule_by_hand():
    """9 x 9, one row: two equal peaks 3 apart on a ridge and a faint bump 3 further on.  T_hi = 4.5, T_lo = 0.5."""
    img = np.zeros((9, 9))
    img[1, :] = [1.0, 5.0, 2.0, 2.0, 5.0, 1.0, 1.0, 3.0, 1.0]  # cells 9 .. 17: peaks at 10 and 13, a faint summit at 16
    kw = dict(thr=(4.5, 0.5), nsigma=(0.0, 0.0), correct=False)
    T_hi, T_lo, P, reason, ll, K = sources_ref.islands(img, **{k: v for k, v in kw.items() if k != "correct"})
    assert reason == 0 and K.sum() == 9
    sub = deblend_ref.basins(img, ll, K, T_hi, 2)[1]
    # 11 climbs to 10, 12 and 14 to 13, 15 and 17 to 16; the faint summit 16 hangs below the brightest cell, 10
    assert sub.tolist() == [10, 10, 10, 13, 13, 13, 10, 10, 10]
    # r = 3: the window of 13 holds 10, equal and of smaller index; that of 16 holds 13, itself no peak: two hops
    assert deblend_ref.basins(img, ll, K, T_hi, 3)[1].tolist() == [10] * 9
    got = deblend_ref.find_sources(img, THETA, 2, **kw)
    assert got["count"] == 2 and got["info"][:, 1].tolist() == [6.0, 3.0] and got["info"][:, 0].tolist() == [9.0, 9.0]
    assert got["info"][:, 15].astype(int).tolist() == [11, 9]  # a line of cells is a point; the first touches the rim; blended
    assert got["info"][0, 11:15].tolist() == [1.0, 1.0, 0.0, 8.0]  # the first basin's box spans the row
    one = deblend_ref.find_sources(img, THETA, 3, **kw)
    assert one["count"] == 1 and one["info"][0, 15] == 3 and one["info"][0, 1] == 9
