"""Auto-masking on the GPU (gridhip_automask*, gridhip_imager_[ms]deconvolve_automask_dev) against tests/automask_ref.py: the
mask byte for byte and the stats bit for bit - nothing is summed, so no tolerance is needed.  The shapes are the smallest
at which the labelling can go wrong, built around the tile of csrc/automask.hip (tests/automask_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import automask_cases
import automask_ref
import noise_ref
from test_automask_host import EINVAL_CASES
from test_gpu_imager import Case, host, to_dev

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ref_of(image, mask0, kw):
    kw = dict(kw)
    return automask_ref.automask(image, mask0, kw.pop("noise", None), **kw)


def check(ctx, name, image, mask0, kw):
    want_mask, want_stats = ref_of(image, mask0, kw)
    mask = mask0.copy()
    got_mask, got_stats = ctx.automask(image, mask, **kw)
    assert got_mask is mask
    bad = np.argwhere(got_mask != want_mask)
    assert bad.size == 0, f"{name}: {len(bad)} bytes differ, the first at {bad[0]}; stats {got_stats} for {want_stats}"
    assert same(got_stats, want_stats), f"{name}: stats {got_stats} for {want_stats}"


@pytest.mark.parametrize("N", automask_cases.sizes())
def test_labelling(ctx, N):
    cases = automask_cases.labelling_cases(N)
    assert len(cases) >= 11
    for name, image, mask0, kw in cases:
        check(ctx, f"N = {N}, {name}", image, mask0, kw)


def test_pruning_hysteresis_growing_accumulation_and_non_finite_cells(ctx):
    for name, image, mask0, kw in automask_cases.feature_cases():
        check(ctx, name, image, mask0, kw)


def sky(N, seed, nsrc=12, sigma=0.01):
    """white noise with a few Gaussian islands of different sizes and signs"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:N, 0:N]
    img = sigma * rng.normal(size=(N, N))
    for _ in range(nsrc):
        y, x, a, w = rng.integers(0, N), rng.integers(0, N), rng.uniform(-1.0, 1.0), rng.uniform(0.7, 4.0)
        img += a * np.exp(-0.5 * ((yy - y) ** 2 + (xx - x) ** 2) / w ** 2)
    return img


def test_many_tiles_at_once(ctx):
    """257 x 257: 9 x 9 tiles, the last of one row and one column; a site percolation near its threshold gives components
    that wander over many tiles, a hundredth of the cells are seeds."""
    N = 257
    rng = np.random.default_rng(5)
    zero = np.zeros((N, N), dtype=np.uint8)
    for p in (0.35, 0.42, 0.5):
        inset = rng.random((N, N)) < p
        img = inset.astype(np.float64)
        img[rng.random((N, N)) < 0.01] += 1.0
        check(ctx, f"percolation {p}", img, zero, dict(thr=(1.5, 0.5), nsigma=(0, 0), min_cells=2, grow=1, border=3))


@pytest.mark.parametrize("absolute", [False, True])
def test_levels_from_image_stats_on_the_device(ctx, absolute):
    th, tw = automask_cases.tile()
    N = 2 * tw + 3
    img = sky(N, 11)
    img[5, 7], img[40, 3] = np.nan, np.inf
    img[20, 50], img[55, 8] = 0.6, -0.7  # two lone cells above T_hi: pruned by min_cells
    dimg = to_dev(img)
    ist = ctx.image_stats(dimg, None, 2)
    assert same(host(ist), noise_ref.image_stats(img, None, 2))
    start = np.zeros((N, N), dtype=np.uint8)
    start[10:12, :] = 5
    dmask = to_dev(start)
    kw = dict(border=2, absolute=absolute, nsigma=(5, 2.5), peak_frac=0.02, min_cells=3, grow=2)
    m, st = ctx.automask(dimg, dmask, ist[3:4], **kw)
    assert m is dmask
    want_mask, want_stats = automask_ref.automask(img, start, float(host(ist)[3]), **kw)
    print(f"absolute {absolute}: stats {host(st)}")
    assert want_stats[4] >= 2 and want_stats[3] > want_stats[4] and want_stats[6] > 0  # something pruned, something kept
    assert np.array_equal(host(m), want_mask) and same(host(st), want_stats)
    assert np.all(host(m)[10:12, :] == 5)


def test_no_usable_sigma_and_nothing_taking_part(ctx):
    N = 40
    img = sky(N, 3)
    start = (np.arange(N * N).reshape(N, N) % 7 == 0).astype(np.uint8) * 9
    dmask = to_dev(start)
    nan_sigma = to_dev(np.array([np.nan]))
    m, st = ctx.automask(to_dev(img), dmask, nan_sigma, nsigma=(5, 2.5), grow=3)
    want_mask, want_stats = automask_ref.automask(img, start, np.nan, nsigma=(5, 2.5), grow=3)
    assert want_stats[7] == 3 and np.array_equal(host(m), start) and same(host(st), want_stats)
    # fixed levels do not read sigma: the same NaN is harmless
    m, st = ctx.automask(to_dev(img), to_dev(start), nan_sigma, nsigma=0, thr=(0.5, 0.1))
    want_mask, want_stats = automask_ref.automask(img, start, np.nan, nsigma=(0, 0), thr=(0.5, 0.1))
    assert want_stats[7] == 0 and np.array_equal(host(m), want_mask) and same(host(st), want_stats)
    allnan = np.full((N, N), np.nan)
    allnan[0, :] = 1.0  # finite cells outside the border region only
    m, st = ctx.automask(to_dev(allnan), dmask, to_dev(np.array([0.5])), border=1)
    want_mask, want_stats = automask_ref.automask(allnan, start, 0.5, border=1)
    assert want_stats[7] == 2 and np.array_equal(host(m), start) and same(host(st), want_stats)
    # NaN sigma and nothing taking part: reason 3 comes first
    m, st = ctx.automask(to_dev(allnan), dmask, nan_sigma, border=1)
    assert host(st)[7] == 3 and np.array_equal(host(m), start)


def test_host_dev_and_imager_forms_twice(ctx):
    import torch
    c = Case(ctx, "simple", 0.1, 640, 600, 31)
    N = c.N
    img = sky(N, 8, sigma=0.02)
    start = np.zeros((N, N), dtype=np.uint8)
    start[3, 4] = 77
    kw = dict(border=1, absolute=True, nsigma=(4, 2), min_cells=2, grow=1)
    sigma = float(noise_ref.image_stats(img, None, 1)[3])
    want_mask, want_stats = automask_ref.automask(img, start, sigma, **kw)
    assert want_stats[5] >= 1
    dimg, dsig = to_dev(img), to_dev(np.array([sigma]))
    outs = []
    for rep in range(2):
        outs.append(ctx.automask(img, start.copy(), sigma, **kw))
        m, s = ctx.automask(dimg, to_dev(start), dsig, **kw)
        outs.append((host(m), host(s)))
        m, s = c.im.automask(dimg, to_dev(start), dsig, **kw)
        outs.append((host(m), host(s)))
        mb, s = c.im.automask(dimg, to_dev(start != 0), dsig, **kw)  # a bool mask: its own bytes
        assert mb.dtype == torch.bool and np.array_equal(host(mb), want_mask != 0)
    for m, s in outs:
        assert np.array_equal(m, want_mask) and same(s, want_stats)
    assert ctx.get_option("errors") == 0
    c.im.close()


def test_stats_automask_and_clean_auto_in_one_graph(ctx):
    import torch
    c = Case(ctx, "simple", 0.1, 640, 600, 41)
    im, N = c.im, c.N
    base = to_dev(sky(N, 9, sigma=0.02))
    kw = dict(border=1, nsigma=(4, 2), min_cells=2, grow=1)
    ckw = dict(gain=0.2, threshold=0.0, niter=20, border=1, patch=0, nsigma=3.0)
    img, model = (torch.zeros((N, N), dtype=torch.float64, device="cuda:0") for _ in range(2))
    mask = torch.zeros((N, N), dtype=torch.uint8, device="cuda:0")

    def work(img, mask, model):
        ist = im.image_stats(img, None, 1)
        _, ast = im.automask(img, mask, ist[3:4], **kw)
        _, _, st = im.clean(img, model, mask=mask, noise=ist[3:4], **ckw)
        return ist, ast, st
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream: the first calls' allocations
        img.copy_(base)
        work(img, mask, model)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = work(img, mask, model)
    torch.cuda.synchronize()
    for rep in range(2):
        img.copy_(base * (rep + 1))
        mask.zero_()
        model.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (img, mask, model, *outs)]
        e_img, e_mask, e_model = base * (rep + 1), torch.zeros_like(mask), torch.zeros_like(model)
        want = work(e_img, e_mask, e_model)
        torch.cuda.synchronize()
        assert got[1].any() and np.count_nonzero(got[2]) > 0
        assert np.array_equal(got[1], host(e_mask))
        for a, b in zip([got[0], got[2], *got[3:]], (e_img, e_model, *want)):
            assert same(a, host(b))
    assert ctx.get_option("errors") == 0
    im.close()


LOOP = dict(gain=0.3, threshold=0.0, niter=40, border=2, patch=0, nsigma=3.0, peak_frac=0.05)
LOOP_AM = dict(absolute=False, thr=(0, 0), nsigma=(4.5, 2.5), peak_frac=0.1, min_cells=1, grow=1)


def loop_case(ctx):
    """the sizes tests/test_gpu_noise.py uses for deconvolve_auto, and its random baselines: 6000 visibilities on a
    64 x 64 grid, three to a cell on average after the mirror"""
    from test_gpu_noise import noisy_sky
    c = Case(ctx, "simple", 0.1, 640, 6000, 71)
    vis, _ = noisy_sky(c, 72, amp=3.0)
    return c.im, c.N, vis


def paired_case(ctx):
    """The same sizes - theta 0.1, lam 640 (N = 64), 6000 visibilities - with baselines under which a cycle is the same
    bits on every run, so that a loop can be compared with the calls it replaces bit for bit.  The gridder's scatter adds
    the visibilities of a cell with fp64 atomics in an order the hardware picks, and a sum of three or more doubles
    depends on that order; a sum of two does not.  So every cell of the mirrored stream receives exactly two
    visibilities or none: each of the 1984 cells of the half plane v > 0 (or v = 0, u > 0) inside the grid gets two, at
    random places in the cell and each on a random side of the mirror, and the 2032 that are left lie beyond the grid's
    edge, where the gridder drops them (the random stream has such visibilities too).  A few point sources are predicted
    through the imager and unit noise times 3 is added, as noisy_sky does."""
    import torch
    theta, lam, n, N = 0.1, 640, 6000, 64
    rng = np.random.default_rng(71)
    cells = np.array([(i, j) for j in range(0, N // 2) for i in range(1 - N // 2, N // 2) if j > 0 or i > 0], dtype=np.float64)
    assert len(cells) == 1984
    c2 = np.repeat(cells, 2, axis=0)
    inside = rng.choice([-1.0, 1.0], len(c2))[:, None] * (c2 + rng.uniform(0.05, 0.3, c2.shape)) / N
    nout = n - len(inside)
    outside = np.stack([rng.choice([-1.0, 1.0], nout) * rng.uniform(34.0, 38.0, nout), rng.uniform(-30.0, 30.0, nout)], 1) / N
    p = rng.permutation(np.concatenate([inside, outside]))
    assert p.shape == (n, 2)
    duvw = tuple(to_dev(x) for x in (p[:, 0] * lam, p[:, 1] * lam, rng.uniform(-100.0, 100.0, n)))
    im = ctx.imager(theta, lam, duvw, ("simple",))
    assert im.N == N
    sky = np.zeros((N, N))
    for _ in range(4):
        sky[rng.integers(N // 4, N - N // 4), rng.integers(N // 4, N - N // 4)] = rng.uniform(0.5, 1.0)
    vis = im.predict(to_dev(sky)) + 3.0 * to_dev(rng.normal(size=n) + 1j * rng.normal(size=n))
    torch.cuda.synchronize()
    return im, N, vis, to_dev(sky)


def loop_and_sequence(im, N, vis, scales, nmajor=3):
    """(model, image, mask, stats, istats, astats) of Imager.deconvolve(automask=...) and of the same sequence issued call
    by call, as host arrays"""
    import torch
    kw, am = LOOP, LOOP_AM
    extra = {} if scales is None else dict(scales=scales)
    model, image, stats, istats, mask, astats = im.deconvolve(vis, nmajor, automask=am, **kw, **extra)
    m2 = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    k2 = torch.zeros((N, N), dtype=torch.uint8, device="cuda:0")
    rows, irows, arows = [], [], []
    for cyc in range(nmajor):
        img = im.cycle(vis, m2)
        ist = im.image_stats(img, None, kw["border"])
        _, ast = im.automask(img, k2, ist[3:4], kw["border"], **am)
        if scales is None:
            _, _, s = im.clean(img, m2, mask=k2, noise=ist[3:4], **kw)
        else:
            _, _, s = im.msclean(img, scales, model=m2, mask=k2, noise=ist[3:4], **kw)
        rows.append(host(s))
        irows.append(host(ist))
        arows.append(host(ast))
    closing = im.cycle(vis, m2)
    got = tuple(host(t).copy() for t in (model, image, mask, stats, istats, astats))
    want = (host(m2), host(closing), host(k2), np.array(rows), np.array(irows), np.array(arows))
    gm, gi, gk, gs, gis, gas = got
    print(f"scales {scales}: automask rows {gas.tolist()} iterations {gs[:, 0].tolist()} reasons {gs[:, -3].tolist()}")
    print("model, image, mask, stats, istats, astats differ by at most "
          + ", ".join(f"{np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))):.3e}" for a, b in zip(got, want)))
    assert gk.any() and np.count_nonzero(gm) > 0 and gas[0, 5] >= 1
    assert scales is not None or not gm[gk == 0].any()  # (a delta component lies under the mask)
    return got, want


@pytest.mark.parametrize("scales", [None, [0.0, 3.0]])
def test_deconvolve_automask_is_the_loop_it_replaces(ctx, scales):
    """Imager.deconvolve(automask=...) against the same sequence issued call by call: model, image, mask and the three
    stats tables, bit for bit, on baselines under which `cycle` itself is the same bits on every run (paired_case says
    how; the test first checks that it is, without and with a model)."""
    im, N, vis, sky = paired_case(ctx)
    for model in (None, sky):
        twice = [host(im.cycle(vis, model)).copy() for _ in range(2)]
        assert same(*twice), f"precondition: two cycles of the same input differ by {np.abs(twice[0] - twice[1]).max():.3e}"
    got, want = loop_and_sequence(im, N, vis, scales)
    assert np.array_equal(got[2], want[2])
    for a, b, what in zip(got, want, ("model", "image", "mask", "stats", "istats", "astats")):
        assert same(a, b), what
    im.close()


@pytest.mark.parametrize("scales", [None, [0.0, 3.0]])
def test_deconvolve_automask_on_random_baselines(ctx, scales):
    """The same comparison on the random baselines tests/test_gpu_noise.py uses for deconvolve_auto.  There a cell receives
    three visibilities on average, the order of the gridder's fp64 atomics shows in the last bits of every cycle's image
    (measured: two cycles of the same input differ by 5e-17 to 8e-17), and the loop and the sequence run their cycles
    apart.  So the mask and every count are compared exactly, and the doubles at 1e-10 of the largest value, the
    tolerance tests/test_gpu_noise.py and tests/test_gpu_imager.py compare cycles at (measured here: at most 4.4e-16)."""
    im, N, vis = loop_case(ctx)
    got, want = loop_and_sequence(im, N, vis, scales)
    (gm, gi, gk, gs, gis, gas), (wm, wi, wk, ws, wis, was) = got, want
    assert np.array_equal(gk, wk)
    assert np.array_equal(gas[:, 3:], was[:, 3:]) and np.array_equal(gs[:, 0], ws[:, 0]) and np.array_equal(gs[:, -3], ws[:, -3])
    assert np.array_equal(gis[:, [0, 6]], wis[:, [0, 6]])
    for a, b in ((gm, wm), (gi, wi), (gs, ws), (gis, wis), (gas, was)):
        assert np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), np.abs(wi).max())
    im.close()


@pytest.mark.parametrize("scales", [None, [0.0, 3.0]])
def test_deconvolve_automask_with_nothing_above_the_level(ctx, scales):
    """levels nothing reaches: the mask stays empty, the model stays zero and every stats row carries clean_auto's reason
    2, while every cycle still images and measures"""
    im, N, vis = loop_case(ctx)
    extra = {} if scales is None else dict(scales=scales)
    high = dict(LOOP_AM, thr=(1e6, 1e6))
    model, image, stats, istats, mask, astats = im.deconvolve(vis, 3, automask=high, **LOOP, **extra)
    gs, gas = host(stats), host(astats)
    assert not host(mask).any() and not host(model).any()
    assert np.all(gs[:, -3] == 2) and np.all(gs[:, 0] == 0)
    assert np.all(gas[:, 3:] == 0) and np.all(gas[:, 0] == 1e6) and np.all(gas[:, 2] > 0)
    assert np.all(host(istats)[:, 0] == (N - 4) ** 2) and np.all(host(istats)[:, 3] > 0)
    assert np.abs(host(image)).max() > 0
    im.close()


def test_refusals(ctx):
    """every argument the header refuses, with a context, in the host and the _dev form: the code, and nothing touched"""
    import torch
    import gridhip
    EINVAL, EUNSUPPORTED = gridhip._lib.EINVAL, gridhip._lib.EUNSUPPORTED
    N = 8
    img = torch.full((N * N,), 1.5, dtype=torch.float64, device="cuda:0")
    mask = torch.full((N * N,), 5, dtype=torch.uint8, device="cuda:0")
    stats = torch.full((8,), 7.0, dtype=torch.float64, device="cuda:0")
    noise = torch.full((1,), 9.0, dtype=torch.float64, device="cuda:0")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    base = dict(N=N, image=p(img), mask=p(mask), border=0, absolute=0, thr_hi=1.0, thr_lo=0.5, nsigma_hi=5.0,
                nsigma_lo=2.5, noise=p(noise), peak_frac=0.1, min_cells=1, grow=1, stats=p(stats))
    order = ("N", "image", "mask", "border", "absolute", "thr_hi", "thr_lo", "nsigma_hi", "nsigma_lo", "noise", "peak_frac",
             "min_cells", "grow", "stats")
    lib, h = ctx._lib, ctx._h
    ctx._use_torch_stream()
    c = Case(ctx, "simple", 0.1, 80, 50, 3)  # an imager of N = 8
    assert c.N == N
    overlaps = [dict(mask=p(img)), dict(mask=p(img, N * N * 8 - 1)), dict(stats=p(img, 8)), dict(stats=p(mask, 0))]
    for change, code in ([(x, EINVAL) for x in EINVAL_CASES + overlaps]
                         + [(dict(grow=33), EUNSUPPORTED), (dict(N=46341), EUNSUPPORTED),
                            (dict(grow=33, min_cells=0), EINVAL)]):
        args = [dict(base, **change)[k] for k in order]
        assert lib.gridhip_automask_dev(h, *args) == code, change
        assert lib.gridhip_automask(h, *args) == code, change
        if "N" not in change:
            assert lib.gridhip_imager_automask_dev(c.im._h, *args[1:]) == code, change
    # the loop refuses what the calls it replaces refuse, before anything is enqueued
    vis = torch.zeros(c.im.n, dtype=torch.complex128, device="cuda:0")
    model = torch.full((N * N,), 2.5, dtype=torch.float64, device="cuda:0")
    cl = (0.1, 0.0, 5, 0, 0)
    ok = (p(mask), 3.0, 0.1, 0, 1.0, 0.5, 5.0, 2.5, 0.1, 1, 1, p(stats), None, None)
    for i, v in ((0, None), (1, -1.0), (2, 1.0), (4, 0.25), (7, 6.0), (8, 1.0), (9, 0), (10, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.gridhip_imager_deconvolve_automask_dev(c.im._h, p(vis), p(model), p(img), 2, *cl, *bad) == EINVAL, (i, v)
    bad = list(ok)
    bad[10] = 33
    assert lib.gridhip_imager_deconvolve_automask_dev(c.im._h, p(vis), p(model), p(img), 2, *cl, *bad) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(img == 1.5) and torch.all(mask == 5) and torch.all(stats == 7.0) and torch.all(model == 2.5)
    assert noise[0] == 9.0
    c.im.close()
