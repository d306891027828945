"""Deblending in the source finder on the GPU (option "sources_deblend", Context.find_sources(deblend=r)) against
tests/deblend_ref.py.  What is exact - the island's label, ncells, the peak's cell, the box, the flags, the count and the
order of the rows - is compared bit for bit, and on images of small integers, whose sums are exact, so is everything else; on
arbitrary values the sums lie within test_gpu_sources' bound on two summation orders and the derived fields are recomputed
from the GPU's own sums.  N is 5 to 33, but for the forms and the graph, which take test_gpu_sources' own 64 x 64 sky.
Every case is a function of a context: test_on_filled_scratch runs them again on contexts whose scratch starts as 0xFF and
0x01 bytes (but the captured one: a fill is a memset node, include/gridhip.h "scratch_fill")."""
import math

import numpy as np
import pytest

import deblend_ref
import noise_ref
import test_gpu_sources as tgs
from test_deblend_host import KW as PAIR_KW, pair_image
from test_gpu_imager import Case, host, to_dev
from test_sources_host import beam_of, gaussian_covariance

pytestmark = pytest.mark.gpu

THETA, FIXED, EXACT = tgs.THETA, tgs.FIXED, tgs.EXACT
BLENDED = deblend_ref.BLENDED


def ref_of(image, r, kw, beam=None, max_c=None):
    kw = dict(kw)
    return deblend_ref.find_sources(image, THETA, r, kw.pop("noise", None), beam=beam, max_c=max_c, **kw)


def check(ctx, name, image, r, kw, exact=True, beam=None, rows=None):
    """the host form against the restatement; rows: the number of rows the case is built to give"""
    N = image.shape[0]
    want = ref_of(image, r, kw, beam)
    n = want["count"]
    assert rows is None or n == rows, f"{name}: the restatement finds {n} rows, the case is built for {rows}"
    out = np.full((n + 2, 10), -7.0)
    comps, count, info, stats = ctx.find_sources(THETA, tgs.lam_of(N), image, beam, max_sources=n + 2, out=out, deblend=r, **kw)
    print(f"{name}: r = {r}, {count} rows for {n}, peaks {info[:count, 2:4].astype(int).tolist()}, flags "
          f"{info[:count, 15].astype(int).tolist()}")
    assert comps is out and count == n, f"{name}: {count} rows for {n}"
    assert tgs.same(info[:n, EXACT], want["info"][:, EXACT]), (name, info[:n, EXACT], want["info"][:, EXACT])
    assert np.array_equal(info[:n, 15], want["info"][:, 15]), (name, info[:n, 15], want["info"][:, 15])
    assert tgs.same(stats[:5], want["stats"][:5]) and stats[7] == 0, name
    assert np.all(comps[n:] == -7.0) and np.all(info[n:] == 0.0), name
    if exact:
        for got, ref, what in ((comps[:n], want["comps"], "comps"), (info[:n], want["info"], "info"), (stats, want["stats"], "stats")):
            assert tgs.same(got, ref), f"{name}: {what} differs: {got!r} for {ref!r}"
    else:
        ok, worst = tgs.within_sum_bound(info[:n], want)
        print(f"  the worst sum at {worst:.3f} of its bound")
        assert ok, (name, worst)
        plain = info[:n].copy()
        plain[:, 15] = plain[:, 15].astype(int) & ~BLENDED  # (check_derived compares the flags with derive's)
        tgs.check_derived(comps[:n], plain, stats[1], N, kw.get("border", 0), beam, kw.get("correct", True))
    return comps[:n], info[:n], stats


def levels(hi, lo, **kw):
    return dict(thr=(hi, lo), correct=False, **FIXED, **kw)


# ---- the cases: each a function of a context ---------------------------------------------------------------------------------
def case_blended_pair(ctx):
    """the issue's pair: two rows at every r, near the true positions, sharing the island's label, both flagged"""
    img = pair_image()
    for r in (1, 2, 4):
        comps, info, stats = check(ctx, "pair", img, r, dict(PAIR_KW, noise=None), exact=False, rows=2)
        assert info[0, 0] == info[1, 0] and np.all(info[:, 15].astype(int) & BLENDED)
    check(ctx, "pair, corrected, beam", img, 2, dict(PAIR_KW, noise=None, correct=True), exact=False,
          beam=np.array(beam_of(gaussian_covariance(3.0, 2.0, 0.4))), rows=2)


def case_equal_peaks_r_and_r_plus_1_apart(ctx):
    """r apart: the second is in the first's window and the other way round; the smaller index wins.  r + 1: two rows."""
    r = 3
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        for d, rows in ((r, 1), (r + 1, 2)):
            img = np.zeros((17, 17))
            img[2:15, 2:15] = 1.0
            y0, x0 = 4, (4 if dx >= 0 else 12)
            img[y0, x0] = img[y0 + d * dy, x0 + d * dx] = 5.0
            comps, info, stats = check(ctx, f"equal peaks {d} apart along ({dy}, {dx})", img, r, levels(2.5, 0.5), rows=rows)
            assert (info[0, 2], info[0, 3]) == (y0, x0)
            assert np.all((info[:, 15].astype(int) & BLENDED != 0) == (rows == 2))


def case_plateau(ctx):
    """two cells of the peak's value side by side: one peak, the smaller index; and a second peak to split from"""
    img = np.zeros((16, 16))
    img[3:12, 2:14] = 1.0
    img[5, 5] = img[5, 6] = 4.0
    check(ctx, "a two-cell plateau", img, 2, levels(2.5, 0.5), rows=1)
    img[9, 11] = 3.0
    img[9, 10] = 3.0
    comps, info, stats = check(ctx, "two plateaus", img, 2, levels(2.5, 0.5), rows=2)
    assert info[:, 2:4].tolist() == [[5.0, 5.0], [9.0, 10.0]]


def case_other_island_in_the_window(ctx):
    """a summit whose window holds a brighter cell of another island: it stays a peak"""
    img = np.zeros((12, 12))
    img[5, 2:5] = [1.0, 3.0, 1.0]
    img[5, 6:9] = [1.0, 9.0, 1.0]
    img[7, 2:5] = [1.0, 2.0, 1.0]
    img[6, 4] = 1.0  # a second summit of the first island, whose window holds the 3 of its own island and the 9 as well
    comps, info, stats = check(ctx, "another island in the window", img, 4, levels(2.5, 0.5), rows=2)
    assert not np.any(info[:, 15].astype(int) & BLENDED)
    assert info[:, 2:4].tolist() == [[5.0, 3.0], [5.0, 7.0]] and info[0, 1] == 7


def case_corner(ctx):
    """summits in the image's corners: the window is clipped at two sides"""
    N = 9
    img = np.zeros((N, N))
    img[0:2, :] = 1.0
    img[:, 0:2] = 1.0
    img[N - 2:, :] = 1.0
    img[:, N - 2:] = 1.0
    img[0, 0], img[0, N - 1], img[N - 1, 0], img[N - 1, N - 1] = 5.0, 6.0, 7.0, 8.0
    img[0, 4] = 3.0
    for r, rows in ((2, 5), (4, 4), (8, 1)):
        check(ctx, "corners", img, r, levels(2.5, 0.5), rows=rows)
    check(ctx, "corners, border 1", img, 2, levels(0.75, 0.5, border=1), rows=1)


ROW = [1.0, 5.0, 2.0, 2.0, 5.0, 1.0, 1.0, 3.0, 1.0]  # test_deblend_host.test_the_rule_by_hand


def case_faint_summit(ctx):
    """r = 2: the bump of 3 <= T_hi at the end is a summit of its own window; its cells go to the brightest peak's row"""
    img = np.zeros((9, 9))
    img[1, :] = ROW
    comps, info, stats = check(ctx, "a faint summit", img, 2, levels(4.5, 0.5), rows=2)
    assert info[:, 1].tolist() == [6.0, 3.0] and info[0, 11:15].tolist() == [1.0, 1.0, 0.0, 8.0]
    img[1, 4] = 6.0  # now the second peak is the brightest: the bump's cells are its
    comps, info, stats = check(ctx, "a faint summit, the later peak the brightest", img, 2, levels(4.5, 0.5), rows=2)
    assert info[:, 1].tolist() == [3.0, 6.0]


def case_two_hops(ctx):
    """r = 3: the bump's window holds the second 5, which itself climbs on to the first"""
    img = np.zeros((9, 9))
    img[1, :] = ROW
    comps, info, stats = check(ctx, "two hops", img, 3, levels(4.5, 0.5), rows=1)
    assert info[0, 1] == 9 and int(info[0, 15]) & BLENDED == 0


def spiral(N):
    path, seen = [], set()
    y = x = 0
    dy, dx = 0, 1
    inside = lambda p: 0 <= p[0] < N and 0 <= p[1] < N  # noqa: E731
    while True:
        path.append((y, x))
        seen.add((y, x))
        if not inside((y + dy, x + dx)) or (y + 2 * dy, x + 2 * dx) in seen:
            dy, dx = dx, -dy
            if not inside((y + dy, x + dx)) or (y + dy, x + dx) in seen or (y + 2 * dy, x + 2 * dx) in seen:
                return path
        y, x = y + dy, x + dx


def case_spiral_ridge(ctx):
    """a one-cell-wide ridge that winds inwards and rises by 1 per cell: the ascent of the outermost cell is as long as the
    ridge (but for the corners it cuts), and ends: one row"""
    N = 33
    path = spiral(N)
    assert len(path) > 500
    img = np.zeros((N, N))
    for i, (y, x) in enumerate(path):
        img[y, x] = 1.0 + i
    comps, info, stats = check(ctx, "a spiral ridge", img, 2, levels(2.5, 0.5), rows=1)
    assert info[0, 1] == len(path) and (info[0, 2], info[0, 3]) == path[-1]
    down = np.zeros((N, N))  # the other way: the summit is the first cell, every pointer goes to a smaller index
    for i, (y, x) in enumerate(path):
        down[y, x] = float(len(path) - i)
    comps, info, stats = check(ctx, "a spiral ridge, falling", down, 1, levels(2.5, 0.5), rows=1)
    assert (info[0, 2], info[0, 3]) == (0, 0)


def case_r32_on_n5(ctx):
    img = np.ones((5, 5))
    img[0, 0], img[4, 4], img[2, 2] = 5.0, 6.0, 4.0
    check(ctx, "r = 32 on N = 5", img, 32, levels(2.5, 0.5), rows=1)
    check(ctx, "r = 1 on N = 5", img, 1, levels(2.5, 0.5), rows=3)


def three_peaks():
    img = np.zeros((20, 20))
    img[2:18, 2:18] = 1.0
    img[4, 4], img[9, 12], img[15, 5] = 5.0, 7.0, 6.0
    return img


def case_fewer_rows_than_components(ctx):
    """max_c = 2 of 3: the count is 3, two rows are written, what lies after them stays; max_c = 0: counted, no row"""
    import torch
    img, kw = three_peaks(), levels(2.5, 0.5)
    N = img.shape[0]
    full = ref_of(img, 3, kw)
    assert full["count"] == 3
    want = ref_of(img, 3, kw, max_c=2)
    block = torch.full((4, 10), -7.0, dtype=torch.float64, device="cuda:0")
    dc, dn, di, ds = ctx.find_sources(THETA, tgs.lam_of(N), to_dev(img), max_sources=2, out=block[:2], deblend=3, **kw)
    assert int(host(dn)[0]) == 3
    assert tgs.same(host(dc), want["comps"]) and tgs.same(host(di), want["info"]) and np.all(host(block)[2:] == -7.0)
    assert tgs.same(host(ds), want["stats"]) and host(ds)[3] == 3 and host(ds)[4] == 2
    out = np.full((4, 10), -7.0)
    c, n, i, s = ctx.find_sources(THETA, tgs.lam_of(N), img, max_sources=2, out=out[:2], deblend=3, **kw)
    assert n == 3 and tgs.same(c, want["comps"]) and tgs.same(i, want["info"]) and np.all(out[2:] == -7.0)
    want = ref_of(img, 3, kw, max_c=0)
    for image in (img, to_dev(img)):
        c, n, i, s = ctx.find_sources(THETA, tgs.lam_of(N), image, max_sources=0, deblend=3, **kw)
        n, s = (n, s) if isinstance(n, int) else (int(host(n)[0]), host(s))
        assert n == 3 and tgs.same(s, want["stats"]) and s[4] == 0 and tuple(c.shape) == (0, 10)


def case_no_island(ctx):
    """reasons 3 and 2 and a level above everything, after a call that left planes behind: count 0, nothing written"""
    img = three_peaks()
    N = img.shape[0]
    lam = tgs.lam_of(N)
    ctx.find_sources(THETA, lam, to_dev(img), max_sources=4, deblend=2, **levels(2.5, 0.5))
    sentinel = lambda: to_dev(np.full((4, 10), -7.0))  # noqa: E731
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), None, to_dev(np.array([np.nan])), max_sources=4, out=out, deblend=2)
    want = ref_of(img, 2, dict(noise=np.nan))
    assert want["stats"][7] == 3 and tgs.same(host(s), want["stats"]) and int(host(n)[0]) == 0 and np.all(host(out) == -7.0)
    allnan = np.full((N, N), np.nan)
    allnan[0, :] = 1.0
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(allnan), None, to_dev(np.array([0.5])), border=1, max_sources=4, out=out,
                                  deblend=2)
    want = ref_of(allnan, 2, dict(noise=0.5, border=1))
    assert want["stats"][7] == 2 and tgs.same(host(s), want["stats"]) and int(host(n)[0]) == 0 and np.all(host(out) == -7.0)
    c, n, i, s = ctx.find_sources(THETA, lam, allnan, None, 0.5, border=1, max_sources=4, deblend=2)
    assert n == 0 and tgs.same(s, want["stats"]) and not c.any()
    kw = dict(thr=(1e6, 1e6), **FIXED)
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), max_sources=4, out=out, deblend=2, **kw)
    assert int(host(n)[0]) == 0 and tgs.same(host(s), ref_of(img, 2, kw)["stats"]) and np.all(host(out) == -7.0)


def case_single_peaks_equal_the_option_off(ctx):
    """islands of one peak each, in arbitrary values, with a beam and the correction: the bits of the option off"""
    N = 33
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    img = 3.0 * np.exp(-((xx - 9.3) ** 2 / 8.0 + (yy - 8.6) ** 2 / 5.0)) + 2.0 * np.exp(-((xx - 22.7) ** 2 + (yy - 24.1) ** 2) / 6.0)
    beam = np.array(beam_of(gaussian_covariance(2.0, 1.5, 0.3)))
    kw = dict(thr=(0.5, 0.05), correct=True, **FIXED)
    a = ctx.find_sources(THETA, tgs.lam_of(N), img, beam, max_sources=4, **kw)
    assert a[1] == 2
    for r in (1, 4):
        b = ctx.find_sources(THETA, tgs.lam_of(N), img, beam, max_sources=4, deblend=r, **kw)
        assert b[1] == 2 and tgs.same(a[0], b[0]) and tgs.same(a[2], b[2]) and tgs.same(a[3], b[3])


def sky(N=64, seed=37):
    beamcov = gaussian_covariance(3.0, 2.0, math.radians(-35.0))
    return tgs.sky_case(67, seed, beamcov)[:N, :N].copy(), np.array(beam_of(beamcov))


def case_forms_twice(ctx):
    """the host, _dev and imager forms, each twice: the same bits, and the restatement's exact fields"""
    c = Case(ctx, "simple", 0.1, 640, 600, 31)
    assert c.N == 64
    img, beam = sky()
    sigma = float(noise_ref.image_stats(img, None, 1)[3])
    kw = dict(border=1, nsigma=(5, 2.5), min_cells=2, correct=True, max_sources=16, deblend=2)
    dimg, dsig, dbeam = to_dev(img), to_dev(np.array([sigma])), to_dev(beam)
    outs = []
    for rep in range(2):
        a = ctx.find_sources(THETA, 640, img, beam, sigma, **kw)
        outs.append((a[0], a[1], a[2], a[3]))
        for b in (ctx.find_sources(THETA, 640, dimg, dbeam, dsig, **kw), c.im.find_sources(dimg, dbeam, dsig, **kw)):
            outs.append((host(b[0]), int(host(b[1])[0]), host(b[2]), host(b[3])))
    first = outs[0]
    for o in outs[1:]:
        assert o[1] == first[1] and tgs.same(o[0], first[0]) and tgs.same(o[2], first[2]) and tgs.same(o[3], first[3])
    want = ref_of(img, 2, dict(border=1, nsigma=(5, 2.5), min_cells=2, correct=True, noise=sigma), beam)
    off = ctx.find_sources(THETA, 640, img, beam, sigma, **dict(kw, deblend=0))
    print(f"{first[1]} rows with r = 2 for {off[1]} islands; flags {first[2][:first[1], 15].astype(int).tolist()}")
    assert first[1] == want["count"] > off[1] >= 3  # (the sky's blended pair is split)
    n = first[1]
    assert tgs.same(first[2][:n, EXACT], want["info"][:, EXACT]) and np.array_equal(first[2][:n, 15], want["info"][:, 15])
    ok, worst = tgs.within_sum_bound(first[2][:n], want)
    assert ok, worst
    assert ctx.get_option("errors") == 0 and ctx.get_option("sources_deblend") == 0
    c.im.close()


def case_refused_above_32(ctx):
    """deblend = 33: GRIDHIP_EINVAL from the three forms, the outputs as they were, the option as it was"""
    import torch
    import gridhip
    c = Case(ctx, "simple", 0.1, 640, 600, 31)
    img, beam = sky()
    dimg = to_dev(img)
    kw = dict(thr=(0.05, 0.02), max_sources=4, deblend=33, **FIXED)
    for dev, call in ((False, lambda o: ctx.find_sources(THETA, 640, img, out=o, **kw)),
                      (True, lambda o: ctx.find_sources(THETA, 640, dimg, out=o, **kw)),
                      (True, lambda o: c.im.find_sources(dimg, out=o, **kw))):
        out = np.full((4, 10), -7.0)
        out = to_dev(out) if dev else out
        with pytest.raises(gridhip.GridHipError) as e:
            call(out)
        assert e.value.code == gridhip._lib.EINVAL and np.all((host(out) if dev else out) == -7.0)
        assert ctx.get_option("sources_deblend") == 0
    # through the ABI, with every output a sentinel on the device
    f = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda:0")  # noqa: E731
    comps, info, stats = f(40, 3.0), f(64, 4.0), f(8, 7.0)
    count = torch.full((1,), 6, dtype=torch.int64, device="cuda:0")
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = [p(dimg), 0, 0.05, 0.02, 0.0, 0.0, None, 0.0, 1, None, 1, 4, p(comps), p(info), p(count), p(stats)]
    ctx._use_torch_stream()
    ctx.set_option("sources_deblend", 33)
    try:
        assert ctx.get_option("sources_deblend") == 33  # set_option stays generic
        assert ctx._lib.gridhip_find_sources_dev(ctx._h, 0.1, 640, *args) == gridhip._lib.EINVAL
        assert ctx._lib.gridhip_find_sources(ctx._h, 0.1, 640, *args) == gridhip._lib.EINVAL
        assert ctx._lib.gridhip_imager_find_sources_dev(c.im._h, *args) == gridhip._lib.EINVAL
    finally:
        ctx.set_option("sources_deblend", 0)
    torch.cuda.synchronize()
    assert torch.all(comps == 3.0) and torch.all(info == 4.0) and count[0] == 6 and torch.all(stats == 7.0)
    c.im.close()


def case_option_reads_back(ctx):
    """find_sources(deblend=2) leaves the option as it found it - 0, or what the caller had set - also when it raises"""
    img, kw = three_peaks(), levels(2.5, 0.5)
    lam = tgs.lam_of(img.shape[0])
    assert ctx.get_option("sources_deblend") == 0
    assert ctx.find_sources(THETA, lam, img, max_sources=4, deblend=2, **kw)[1] == 3
    assert ctx.get_option("sources_deblend") == 0
    ctx.set_option("sources_deblend", 32)
    try:
        assert ctx.find_sources(THETA, lam, img, max_sources=4, deblend=2, **kw)[1] == 3
        assert ctx.get_option("sources_deblend") == 32
        assert ctx.find_sources(THETA, lam, img, max_sources=4, **kw)[1] == 1  # deblend=0 leaves the option alone: r = 32
        with pytest.raises(Exception):
            ctx.find_sources(THETA, lam, img, max_sources=4, deblend=2, **dict(kw, thr=(0.25, 0.5)))  # (thr_lo > thr_hi)
        assert ctx.get_option("sources_deblend") == 32
    finally:
        ctx.set_option("sources_deblend", 0)
    assert ctx.find_sources(THETA, lam, img, max_sources=4, **kw)[1] == 1


CASES = [case_blended_pair, case_equal_peaks_r_and_r_plus_1_apart, case_plateau, case_other_island_in_the_window, case_corner,
         case_faint_summit, case_two_hops, case_spiral_ridge, case_r32_on_n5, case_fewer_rows_than_components, case_no_island,
         case_single_peaks_equal_the_option_off, case_forms_twice, case_refused_above_32, case_option_reads_back]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_case(ctx, case):
    case(ctx)


def test_stats_find_sources_and_dft_predict_in_one_graph(ctx):
    """image_stats -> find_sources -> dft_predict captured with the option set, replayed on two other images: the bytes of
    the eager calls, and more rows than islands"""
    import torch
    N = 64
    base_np, beam = sky(seed=41)
    dbeam, base = to_dev(beam), to_dev(base_np)
    rng = np.random.default_rng(43)
    uvw = tuple(to_dev(rng.uniform(-300.0, 300.0, 200)) for _ in range(3))
    kw = dict(border=1, nsigma=(5, 2.5), min_cells=2, correct=True, max_sources=16)
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")

    def work(img):
        ist = ctx.image_stats(img, None, 1)
        comps, count, info, st = ctx.find_sources(THETA, 640, img, dbeam, ist[3:4], **kw)
        vis = ctx.dft_predict(uvw, comps, count=count)
        return ist, comps, count, info, st, vis
    ctx.set_option("sources_deblend", 2)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):  # warm-up on the capture stream: the first calls' allocations
            img.copy_(base)
            work(img)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            outs = work(img)
        torch.cuda.synchronize()
        for rep in range(2):
            new = base * (rep + 1) if rep == 0 else torch.flip(base, (0,)).contiguous() * 1.5
            img.copy_(new)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            got = [host(t).copy() for t in outs]
            want = work(new.clone())
            torch.cuda.synchronize()
            assert got[2][0] >= 3 and np.abs(got[5]).max() > 0
            assert np.any(got[3][:got[2][0], 15].astype(int) & BLENDED)  # the sky's blended pair is split
            for a, b in zip(got, want):
                b = host(b)
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    finally:
        ctx.set_option("sources_deblend", 0)
    assert ctx.get_option("errors") == 0


@pytest.mark.parametrize("fill", [0xFF, 0x01], ids=lambda b: f"fill{b:02X}")
def test_on_filled_scratch(fill):
    """every case again on a context whose blocks all start as `fill` bytes: a kernel that reads a plane it never wrote shows"""
    import gridhip
    filled = gridhip.Context(0)
    try:
        filled.set_option("scratch_fill", fill)  # before the context's first call
        before = filled.get_option("scratch_filled")
        for case in CASES:
            case(filled)
        assert filled.get_option("scratch_filled") > before
    finally:
        filled.close()
