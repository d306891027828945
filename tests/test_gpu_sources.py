"""Source finding on the GPU (gridhip_find_sources*) against tests/sources_ref.py.  What is exact - the islands, their order,
the counts, boxes and peaks, and every sum of an image of small integers - is compared bit for bit; a sum of arbitrary
values within the first-order bound on two summation orders; the derived fields, recomputed in numpy from the GPU's own
sums, at 1e-12.  The shapes are the smallest at which the labelling and the box walk can go wrong, built around the tile of
csrc/automask.hip (tests/automask_cases.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import automask_cases
import dft_ref
import noise_ref
import sources_ref
from test_gpu_imager import Case, host, to_dev
from test_sources_host import EINVAL_CASES, beam_of, convolved_gaussian, gaussian_covariance

pytestmark = pytest.mark.gpu

THETA = 0.1
FIXED = dict(nsigma=(0.0, 0.0), noise=None)
EXACT = [0, 1, 2, 3, 4, 11, 12, 13, 14]  # label, ncells, yp, xp, P_i, y0, y1, x0, x1 of an info row
SUMS = [5, 6, 7, 8, 9, 10]               # S, Sx, Sy, Sxx, Sxy, Syy


def lam_of(N):
    return 10 * N  # image_size(0.1, 10 N) = N


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ref_of(image, kw, beam=None, max_c=None):
    kw = dict(kw)
    kw.pop("max_sources", None)
    return sources_ref.find_sources(image, THETA, kw.pop("noise", None), beam=beam, max_c=max_c, **kw)


def check_exact(ctx, name, image, kw, beam=None):
    """the host form on an image whose sums are exact: everything bit for bit, and the rows past the count untouched"""
    N = image.shape[0]
    want = ref_of(image, kw, beam)
    rows = want["count"]
    out = np.full((rows + 2, 10), -7.0)
    comps, count, info, stats = ctx.find_sources(THETA, lam_of(N), image, beam, max_sources=rows + 2, out=out, **kw)
    assert comps is out and count == rows, f"{name}: {count} islands for {rows}"
    for got, ref, what in ((comps[:rows], want["comps"], "comps"), (info[:rows], want["info"], "info"),
                           (stats, want["stats"], "stats")):
        if not same(got, ref):
            bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64))
            i = tuple(bad[0])
            raise AssertionError(f"{name}: {what} differs in {len(bad)} places, the first at {i}: {got[i]!r} for {ref[i]!r}")
    assert np.all(comps[rows:] == -7.0) and np.all(info[rows:] == 0.0), name


def box_cases(N):
    """what the box walk can get wrong, in small integers so that every sum is exact: nested boxes, interleaved boxes, a
    peak value that occurs twice, an island on the rim cut by a border"""
    cases = []
    if N < 16:
        return cases
    ring = np.zeros((N, N))
    ring[2:11, 2:11] = 1.0
    ring[3:10, 3:10] = 0.0
    ring[5:8, 5:8] = 2.0  # a blob inside the ring, not touching it
    ring[6, 6] = 5.0
    cases.append(("a ring around a blob", ring, dict(thr=(0.5, 0.5), **FIXED)))
    two = np.zeros((N, N))  # two L shapes whose boxes are the same square
    two[2, 2:9] = two[2:9, 2] = 3.0
    two[8, 4:9] = two[4:9, 8] = 2.0
    two[8, 8] = 4.0
    cases.append(("interleaved boxes", two, dict(thr=(0.5, 0.5), **FIXED)))
    twice = np.zeros((N, N))
    twice[4, 3:9] = [1.0, 3.0, 2.0, 3.0, 1.0, 1.0]
    twice[5, 3:9] = [1.0, 1.0, 1.0, 1.0, 3.0, 1.0]
    cases.append(("the peak value occurs three times", twice, dict(thr=(0.5, 0.5), **FIXED)))
    cases.append(("the same, the peaks alone above T_hi", twice, dict(thr=(2.5, 0.5), min_cells=1, **FIXED)))
    rim = np.zeros((N, N))
    rim[5:8, 0:6] = 1.0
    rim[6, 3] = 2.0
    rim[N - 1, N - 4:N] = 1.0
    rim[N // 2, N // 2] = 1.0
    for border in (0, 2, 3):
        cases.append((f"on the rim, border {border}", rim, dict(thr=(0.5, 0.5), border=border, **FIXED)))
    return cases


@pytest.mark.parametrize("N", automask_cases.sizes() + [257])
def test_patterns_bit_for_bit(ctx, N):
    """automask_cases.patterns(N) as 0/1 images, and the box cases: all sums are exact small integers"""
    pats = automask_cases.patterns(N)
    assert len(pats) >= 5
    for name, inset in pats.items():
        check_exact(ctx, f"N = {N}, {name}", inset.astype(np.float64), dict(thr=(0.5, 0.5), correct=False, **FIXED))
    for name, image, kw in box_cases(N):
        check_exact(ctx, f"N = {N}, {name}", image, dict(kw, correct=False))
    if N >= 16:  # with a beam: a wide one makes points, a narrow one is deconvolved; exact sums still
        for beam in ([0.05, 0.0, 0.05, 0, 0, 0, 8, 1.0], [3.0, 0.5, 2.0, 0, 0, 0, 8, 1.0]):
            for name, image, kw in box_cases(N)[:2]:
                check_exact(ctx, f"N = {N}, {name}, beam {beam[:3]}", image, dict(kw, correct=False), np.array(beam))


def within_sum_bound(info, want):
    """each raw sum within 4 ncells 2^-53 sum |term| of the restatement's: the first-order bound on two summation orders
    of ncells terms (2 (ncells - 1) 2^-53 sum |term|) plus the roundings of the products"""
    n = want["info"][:, 1:2]
    bound = 4.0 * n * 2.0 ** -53 * want["mags"]
    err = np.abs(info[:, SUMS] - want["info"][:, SUMS])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    return bool(np.all(err <= bound)), worst


def check_derived(comps, info, T_lo, N, border, beam, correct):
    """the derived fields recomputed in numpy from the GPU's own sums: l, m, F at 1e-12 relative, the shape as the three
    covariance entries rebuilt from (bmaj, bmin, bpa) at 1e-12 (trace m + trace b)"""
    btrace = 0.0 if beam is None else sum(sources_ref.beam_covariance(beam)[::2])
    for row in range(len(comps)):
        comp, flags, cov = sources_ref.derive(info[row, :15], T_lo, THETA, N, border, beam, correct)
        assert int(info[row, 15]) == flags, row
        for j in (0, 1, 2):
            assert abs(comps[row, j] - comp[j]) <= 1e-12 * abs(comp[j]), (row, j, comps[row, j], comp[j])
        assert np.all(comps[row, [3, 4, 5, 9]] == 0.0)
        got = sources_ref.shape_covariance(*comps[row, 6:9], THETA, N)
        ref = sources_ref.shape_covariance(*comp[6:9], THETA, N)
        scale = (abs(cov[0]) + abs(cov[2]) + 2.0 * btrace) if flags & 1 == 0 else 1.0  # trace i + 2 trace b >= trace m + trace b
        assert max(abs(a - b) for a, b in zip(got, ref)) <= 1e-12 * scale, (row, got, ref)
        if flags & 1:
            assert np.all(comps[row, 6:9] == 0.0)


def test_many_islands_of_arbitrary_values(ctx):
    """257 x 257, a site percolation at p = 0.42 with random positive values: 9 x 9 tiles, islands that wander over many of
    them, boxes that overlap everywhere.  The exact fields bit for bit, the sums within the bound; then fewer rows than
    islands: the count is still the total and the rows after max_c keep what they held."""
    import torch
    N = 257
    rng = np.random.default_rng(17)
    img = np.where(rng.random((N, N)) < 0.42, rng.uniform(0.5, 1.5, (N, N)), 0.0)
    kw = dict(thr=(1.3, 0.25), min_cells=1, border=3, correct=True, **FIXED)
    want = ref_of(img, kw)
    rows = want["count"]
    assert rows > 200 and want["info"][:, 1].max() > 2000 and want["info"][:, 1].min() == 1
    comps, count, info, stats = ctx.find_sources(THETA, lam_of(N), img, max_sources=rows, **kw)
    assert count == rows
    assert same(info[:, EXACT], want["info"][:, EXACT])
    assert np.array_equal(info[:, 15].astype(int) & 2, want["info"][:, 15].astype(int) & 2)  # the edge bit
    ok, worst = within_sum_bound(info, want)
    print(f"{rows} islands, the largest of {int(info[:, 1].max())} cells; the worst sum at {worst:.3f} of its bound")
    assert ok
    assert same(stats[:5], want["stats"][:5]) and stats[7] == 0
    firm = np.array([sources_ref.pd_margin(c) > 1e-6 for c in want["cov"]])  # (a line of cells has a singular covariance)
    assert 100 < np.count_nonzero(firm) < rows
    check_derived(comps[firm], info[firm], stats[1], N, 3, None, True)
    # fewer rows than islands, on the device: a view of a larger block shows what lies after the rows
    max_c = rows // 3
    block = torch.full((max_c + 4, 10), -7.0, dtype=torch.float64, device="cuda:0")
    dc, dn, di, ds = ctx.find_sources(THETA, lam_of(N), to_dev(img), max_sources=max_c, out=block[:max_c], **kw)
    assert int(host(dn)[0]) == rows
    assert same(host(dc), comps[:max_c]) and same(host(di), info[:max_c]) and np.all(host(block)[max_c:] == -7.0)
    s = host(ds)
    assert s[3] == rows and s[4] == max_c and s[5] == np.count_nonzero(info[:max_c, 15].astype(int) & 1)
    flux = 0.0
    for f in comps[:max_c, 2]:
        flux += float(f)
    assert s[6] == flux  # added in row order by one thread
    # and on the host: more rows than islands, the rows after the count untouched
    out = np.full((rows + 3, 10), -7.0)
    c2, n2, i2, s2 = ctx.find_sources(THETA, lam_of(N), img, max_sources=rows + 3, out=out, **kw)
    assert n2 == rows and same(c2[:rows], comps) and np.all(c2[rows:] == -7.0) and same(i2[:rows], info) and same(s2, stats)


def sky_case(N, seed, beamcov):
    """Gaussian sources of different shapes, in units per beam, several straddling the edges of the 32 x 32 labelling tile,
    one pair blended into one island, on white noise; two lone noise cells above T_hi that min_cells prunes"""
    th, tw = automask_cases.tile()
    rng = np.random.default_rng(seed)
    img = 0.01 * rng.normal(size=(N, N))
    srcs = [(tw - 0.3, th + 0.4, 6.0, 3.0, 25.0, 3.0), (tw + 0.2, 12.3, 4.0, 4.0, 0.0, 2.0), (14.6, th - 0.5, 8.0, 2.7, 110.0, 4.0),
            (50.4, 52.2, 3.0, 1.5, 60.0, 1.5), (2 * tw - 0.4, 2 * th + 0.1, 0.0, 0.0, 0.0, 0.8), (20.3, 50.6, 5.0, 2.5, 80.0, 2.5),
            (24.9, 53.2, 3.0, 3.0, 0.0, 1.2)]
    for x, y, fmaj, fmin, ang, flux in srcs:
        intrinsic = gaussian_covariance(fmaj, fmin, math.radians(ang)) if fmaj > 0 else np.zeros((2, 2))
        img += convolved_gaussian(N, flux, intrinsic, beamcov, (x, y))[0]
    img[5, 60], img[60, 5] = 0.08, 0.09
    return img


@pytest.mark.parametrize("correct", [False, True])
def test_a_sky_with_a_fitted_beam_and_the_noise_from_the_device(ctx, correct):
    th, tw = automask_cases.tile()
    N = 2 * tw + 3
    beamcov = gaussian_covariance(3.5, 2.5, math.radians(20.0))
    A, B, Cc = beam_of(beamcov)[:3]
    yy, xx = np.mgrid[0:N, 0:N] - N // 2
    psf = np.exp(-(A * xx * xx + 2.0 * B * xx * yy + Cc * yy * yy))
    img = sky_case(N, 23, beamcov)
    dimg = to_dev(img)
    dbeam = ctx.fit_beam(to_dev(psf), window=6, cut=0.3)
    beam = host(dbeam)
    assert beam[7] == 1.0 and beam[:3] == pytest.approx([A, B, Cc], rel=1e-6)
    ist = ctx.image_stats(dimg, None, 2)
    sigma = float(host(ist)[3])
    assert sigma == float(noise_ref.image_stats(img, None, 2)[3])
    kw = dict(border=2, nsigma=(5.0, 2.5), peak_frac=0.01, min_cells=3, correct=correct)
    dc, dn, di, ds = ctx.find_sources(THETA, lam_of(N), dimg, dbeam, ist[3:4], max_sources=32, **kw)
    comps, count, info, stats = host(dc), int(host(dn)[0]), host(di), host(ds)
    want = ref_of(img, dict(kw, noise=sigma), beam)
    print(f"correct {correct}: stats {stats}\n fluxes {comps[:count, 2]}\n flags {info[:count, 15]}")
    assert count == want["count"] and 6 <= count <= 32  # (the blended pair is one island)
    assert min(sources_ref.pd_margin(c) for c in want["cov"]) > 1e-6
    comps, info = comps[:count], info[:count]
    assert same(info[:, EXACT], want["info"][:, EXACT]) and np.array_equal(info[:, 15], want["info"][:, 15])
    ok, worst = within_sum_bound(info, want)
    assert ok, worst
    assert same(stats[:6], want["stats"][:6]) and stats[7] == 0
    check_derived(comps, info, stats[1], N, 2, beam, correct)
    assert np.count_nonzero(want["info"][:, 15] == 0) >= 4  # Gaussians away from the edge
    # the list predicts as it is, its length never read back
    rng = np.random.default_rng(29)
    n = 200
    u, v = (rng.uniform(-0.5 * N / THETA, 0.5 * N / THETA, n) for _ in range(2))
    w = rng.uniform(-100.0, 100.0, n)
    vis = host(ctx.dft_predict((to_dev(u), to_dev(v), to_dev(w)), dc, count=dn))
    ref = dft_ref.dft_predict(want["comps"], u, v, w)[0]
    err = np.abs(vis - ref).max()
    print(f" dft_predict differs from the restatement's list by {err:.3e}, sum |F| = {np.abs(want['comps'][:, 2]).sum():.3f}")
    assert err <= 1e-10 * np.abs(want["comps"][:, 2]).sum()


def test_host_dev_and_imager_forms_twice(ctx):
    c = Case(ctx, "simple", 0.1, 640, 600, 31)
    N = c.N
    beamcov = gaussian_covariance(3.0, 2.0, math.radians(-35.0))
    beam = np.array(beam_of(beamcov))
    assert N == 64
    img = sky_case(67, 37, beamcov)[:N, :N].copy()
    sigma = float(noise_ref.image_stats(img, None, 1)[3])
    kw = dict(border=1, nsigma=(5, 2.5), min_cells=2, correct=True, max_sources=16)
    dimg, dsig, dbeam = to_dev(img), to_dev(np.array([sigma])), to_dev(beam)
    outs = []
    for rep in range(2):
        a = ctx.find_sources(THETA, 640, img, beam, sigma, **kw)
        outs.append((a[0], a[1], a[2], a[3]))
        for b in (ctx.find_sources(THETA, 640, dimg, dbeam, dsig, **kw), c.im.find_sources(dimg, dbeam, dsig, **kw)):
            outs.append((host(b[0]), int(host(b[1])[0]), host(b[2]), host(b[3])))
    first = outs[0]
    assert 3 <= first[1] <= 16
    for o in outs[1:]:
        assert o[1] == first[1] and same(o[0], first[0]) and same(o[2], first[2]) and same(o[3], first[3])
    want = ref_of(img, dict(kw, noise=sigma), beam)
    assert first[1] == want["count"] and same(first[2][:first[1], EXACT], want["info"][:, EXACT])
    assert ctx.get_option("errors") == 0
    c.im.close()


def test_stats_find_sources_and_dft_predict_in_one_graph(ctx):
    import torch
    N = 64
    beamcov = gaussian_covariance(3.0, 2.0, math.radians(-35.0))
    dbeam = to_dev(np.array(beam_of(beamcov)))
    base = to_dev(sky_case(67, 41, beamcov)[:N, :N].copy())
    rng = np.random.default_rng(43)
    uvw = tuple(to_dev(rng.uniform(-300.0, 300.0, 200)) for _ in range(3))
    kw = dict(border=1, nsigma=(5, 2.5), min_cells=2, correct=True, max_sources=16)
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")

    def work(img):
        ist = ctx.image_stats(img, None, 1)
        comps, count, info, st = ctx.find_sources(THETA, 640, img, dbeam, ist[3:4], **kw)
        vis = ctx.dft_predict(uvw, comps, count=count)
        return ist, comps, count, info, st, vis
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
        for a, b in zip(got, want):
            b = host(b)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert ctx.get_option("errors") == 0


def test_reasons_nothing_found_no_rows_and_an_unusable_beam(ctx):
    import gridhip
    N = 40
    beamcov = gaussian_covariance(3.0, 2.0, 0.3)
    beam = np.array(beam_of(beamcov))
    img = sky_case(67, 47, beamcov)[:N, :N].copy()
    lam = lam_of(N)
    nan_sigma = to_dev(np.array([np.nan]))
    sentinel = lambda: to_dev(np.full((4, 10), -7.0))  # noqa: E731
    # reason 3: sigma is NaN - count 0, nothing written
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), None, nan_sigma, max_sources=4, out=out)
    want = ref_of(img, dict(noise=np.nan))
    assert want["stats"][7] == 3 and same(host(s), want["stats"]) and int(host(n)[0]) == 0 and np.all(host(out) == -7.0)
    # fixed levels do not read sigma
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), None, nan_sigma, nsigma=0, thr=(0.05, 0.02), max_sources=4)
    assert host(s)[7] == 0 and int(host(n)[0]) == ref_of(img, dict(thr=(0.05, 0.02), **FIXED))["count"] > 0
    # reason 2: nothing takes part (finite cells outside the border region only) - after a call that left planes behind
    allnan = np.full((N, N), np.nan)
    allnan[0, :] = 1.0
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(allnan), None, to_dev(np.array([0.5])), border=1, max_sources=4, out=out)
    want = ref_of(allnan, dict(noise=0.5, border=1))
    assert want["stats"][7] == 2 and same(host(s), want["stats"]) and int(host(n)[0]) == 0 and np.all(host(out) == -7.0)
    c, n, i, s = ctx.find_sources(THETA, lam, allnan, None, 0.5, border=1, max_sources=4)
    assert n == 0 and same(s, want["stats"]) and not c.any()
    # nothing above the level: reason 0, no island
    kw = dict(thr=(1e6, 1e6), **FIXED)
    out = sentinel()
    c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), max_sources=4, out=out, **kw)
    assert int(host(n)[0]) == 0 and same(host(s), ref_of(img, kw)["stats"]) and np.all(host(out) == -7.0)
    # max_c = 0: the islands are counted, no row exists
    kw = dict(thr=(0.05, 0.02), **FIXED)
    want = ref_of(img, kw, max_c=0)
    for image in (img, to_dev(img)):
        c, n, i, s = ctx.find_sources(THETA, lam, image, max_sources=0, **kw)
        n, s = (n, s) if isinstance(n, int) else (int(host(n)[0]), host(s))
        assert n == want["count"] > 0 and same(s, want["stats"]) and s[4] == 0 and tuple(c.shape) == (0, 10)
    # an unusable beam on the device: NaN in flux and shape, the positions stand, flag bit 2; the host form refuses it
    good = ctx.find_sources(THETA, lam, to_dev(img), to_dev(beam), max_sources=8, **kw)
    for bad in ([np.nan] * 6 + [2.0, 0.0], [1.0, 2.0, 1.0, 0, 0, 0, 8, 1.0]):
        bad = np.array(bad, dtype=np.float64)
        c, n, i, s = ctx.find_sources(THETA, lam, to_dev(img), to_dev(bad), max_sources=8, **kw)
        c, n, i, s, rows = host(c), int(host(n)[0]), host(i), host(s), min(want["count"], 8)
        assert n == want["count"] and np.all(np.isnan(c[:rows][:, [2, 6, 7, 8]])) and np.all(i[:rows, 15].astype(int) & 4)
        assert not np.any(i[:rows, 15].astype(int) & 1) and same(c[:rows, :2], host(good[0])[:rows, :2])
        assert np.isnan(s[6]) and s[5] == 0 and s[7] == 0
        with pytest.raises(gridhip.GridHipError) as e:
            ctx.find_sources(THETA, lam, img, bad, max_sources=8, **kw)
        assert e.value.code == gridhip._lib.EINVAL


def test_refusals(ctx):
    """every argument the header refuses, with a context, in the three forms: the code, and nothing touched"""
    import torch
    import gridhip
    EINVAL, EUNSUPPORTED = gridhip._lib.EINVAL, gridhip._lib.EUNSUPPORTED
    N, max_c = 8, 4
    f = lambda n, v: torch.full((n,), v, dtype=torch.float64, device="cuda:0")  # noqa: E731
    img, noise, beam, comps, info, stats = f(N * N, 1.5), f(1, 9.0), f(8, 1.0), f(max_c * 10, 3.0), f(max_c * 16, 4.0), f(8, 7.0)
    count = torch.full((1,), 6, dtype=torch.int64, device="cuda:0")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    base = dict(theta=0.1, lam=10 * N, image=p(img), border=0, thr_hi=1.0, thr_lo=0.5, nsigma_hi=5.0, nsigma_lo=2.5,
                noise=p(noise), peak_frac=0.1, min_cells=1, beam=p(beam), correct=1, max_c=max_c, comps=p(comps),
                info=p(info), count=p(count), stats=p(stats))
    order = ("theta", "lam", "image", "border", "thr_hi", "thr_lo", "nsigma_hi", "nsigma_lo", "noise", "peak_frac", "min_cells",
             "beam", "correct", "max_c", "comps", "info", "count", "stats")
    lib, h = ctx._lib, ctx._h
    ctx._use_torch_stream()
    c = Case(ctx, "simple", 0.1, 80, 50, 3)  # an imager of N = 8
    assert c.N == N
    overlaps = [dict(comps=p(img)), dict(comps=p(img, N * N * 8 - 8)), dict(info=p(comps, 8)), dict(stats=p(img, 8)),
                dict(count=p(stats, 56)), dict(stats=p(beam)), dict(count=p(noise)), dict(info=p(stats))]
    for change, code in ([(x, EINVAL) for x in EINVAL_CASES + overlaps]
                         + [(dict(lam=463410), EUNSUPPORTED), (dict(lam=463410, max_c=-1), EINVAL)]):
        args = [dict(base, **change)[k] for k in order]
        assert lib.gridhip_find_sources_dev(h, *args) == code, change
        assert lib.gridhip_find_sources(h, *args) == code, change
        if "lam" not in change:
            assert lib.gridhip_imager_find_sources_dev(c.im._h, *args[2:]) == code, change
    torch.cuda.synchronize()
    assert torch.all(img == 1.5) and noise[0] == 9.0 and torch.all(beam == 1.0) and torch.all(comps == 3.0)
    assert torch.all(info == 4.0) and count[0] == 6 and torch.all(stats == 7.0)
    c.im.close()
