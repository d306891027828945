"""The joint CLEAN on the device (gridhip_jclean[_dev], Context.jclean, gridhip.joint_deconvolve) against the numpy
restatement of include/gridhip.h's definition (tests/jclean_ref.py).

Tolerance and preconditions are test_gpu_mfclean.py's: identical iteration counts, final index, reason and component
positions; models, residuals and stats within 1e-10 of the image's peak (nothing is accumulated with atomics: the
residuals are expected bit for bit, and so are the models, whose fused step the restatement takes too; each figure is
printed before it is asserted).  Precondition, asserted on the restatement alone: over all iterations the relative gap
between the two largest |s| exceeds 1e-8 - with a smaller gap a last-bit difference could legitimately change the
component sequence.  The exact fixtures (tests/jclean_cases.py; tests/test_jclean_host.py shows that no operation of
those runs rounds) and the identity with gridhip_clean_auto are compared bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import jclean_cases as J
import jclean_ref
from clean_edge_cases import same_bits
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-10
GAIN = 0.2
METRIC = ("sum", "sumsq")


def run_ref(psfs, img, weights, metric, **kw):
    res, models, trace = img.copy(), np.zeros_like(img), []
    stats = jclean_ref.jclean(psfs, res, models, weights, metric, kw["gain"], kw["threshold"], kw["niter"], kw["border"],
                              kw["patch"], trace=trace)
    return models, res, stats, trace


def run_dev(ctx, psfs, img, weights, metric, **kw):
    m, r, s = ctx.jclean(to_dev(img), to_dev(psfs), METRIC[metric], weights, **kw)
    return host(m), host(r), host(s)


def compare(got, want, peak, what):
    gm, gr, gs = got
    wm, wr, ws = want[:3]
    assert gs[0] == ws[0], f"{what}: {gs[0]} iterations, the reference {ws[0]}"
    assert gs[2] == ws[2], f"{what}: final peak at {gs[2]}, the reference {ws[2]}"
    assert gs[4] == ws[4], f"{what}: reason {gs[4]}, the reference {ws[4]}"
    assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(wm)), f"{what}: component positions differ"
    # (s, L and s1 of the sumsq metric are squares: in units of the peak's square)
    unit = np.array([peak ** (2 if i in (1, 3, 5) and what.startswith("sumsq") else 1) for i in range(16)])
    errs = (np.abs(gm - wm).max() / peak, np.abs(gr - wr).max() / peak,
            (np.abs(gs - ws) / unit)[[1, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15]].max())
    print(f"{what}: models {errs[0]:.2e} residuals {errs[1]:.2e} stats {errs[2]:.2e}")
    assert max(errs) < TOL, (what, errs)
    assert not gs[6:8].any()
    return errs


SHAPES = [(N, P, Q, m) for N in (256, 255, 600) for P, Q, m in ((1, 1, 0), (2, 2, 0), (4, 1, 1), (3, 3, 1))] + \
         [(N, P, Q, m) for N in (256, 255) for P, Q, m in ((8, 8, 0), (8, 1, 1))]


@pytest.mark.parametrize("patch", [0, 32])
@pytest.mark.parametrize("wide_border", [False, True])
# N: even, odd (the planes' slots are misaligned), several tile rows and columns; one PSF and one per plane; both metrics
@pytest.mark.parametrize("N,P,Q,metric", SHAPES)
def test_against_the_restatement(ctx, N, P, Q, metric, wide_border, patch):
    psfs, img = jclean_ref.make_psfs(N, Q), jclean_ref.make_sky(N, P, Q)
    peak = np.abs(img).max()
    border = N // 8 if wide_border else 0
    weights = jclean_ref.default_weights(METRIC[metric], P)
    mid = jclean_ref.midway_threshold(psfs, img, weights, metric, border, patch)
    worst, bits, smallest = 0.0, True, math.inf
    for threshold, midway in ((0.0, False), (mid, True)):
        for niter in (0, 1, 200):
            kw = dict(gain=GAIN, threshold=threshold, niter=niter, border=border, patch=patch)
            want = run_ref(psfs, img, weights, metric, **kw)
            gaps = [g for _, g in want[3]]
            smallest = min([smallest] + gaps)
            assert not gaps or min(gaps) > 1e-8, f"precondition: smallest gap {min(gaps):.2e} (change the seed)"
            if niter == 200:
                # the two thresholds: one stops the loop midway, the other is never reached
                assert (0 < want[2][0] < niter and want[2][4] == 1) if midway else \
                    (want[2][0] == niter and want[2][4] == 0), want[2]
            got = run_dev(ctx, psfs, img, weights, metric, **kw)
            errs = compare(got, want, peak, f"{METRIC[metric]} N {N} P {P} Q {Q} {kw}")
            worst = max(worst, *errs)
            bits = bits and np.array_equal(got[1], want[1])
    print(f"N {N} P {P} Q {Q} {METRIC[metric]} border {border} patch {patch}: worst {worst:.2e}, smallest gap "
          f"{smallest:.2e}, residuals bit for bit {bits}")


@pytest.mark.parametrize("N", [256, 255])
def test_one_plane_and_the_sum_is_clean_auto_bit_for_bit(ctx, N):
    """IDENTITY: P = 1, metric 0, weights NULL (Context.jclean's default for the sum and one plane is the weight 1)"""
    import torch
    psfs, img = jclean_ref.make_psfs(N, 1), jclean_ref.make_sky(N, 1, 1)
    mask = np.random.default_rng(6).random((N, N)) < 0.6
    sigma = 0.02
    autos = [dict(peak_frac=0.1), dict(mask=mask), dict(nsigma=3.0, noise=sigma), dict(mask=mask, nsigma=3.0, noise=sigma),
             dict(mask=mask, nsigma=2.0, noise=float("nan"))]
    for auto in autos:
        for border, patch in ((0, 0), (N // 8, 32)):
            kw = dict(gain=GAIN, threshold=0.01, niter=150, border=border, patch=patch)
            dev = {k: (to_dev(v) if k == "mask" else to_dev(np.array([v])) if k == "noise" else v) for k, v in auto.items()}
            m1, r1, s1 = (host(t) for t in ctx.clean(to_dev(img[0]), to_dev(psfs[0]), **kw, **dev))
            m2, r2, s2 = (host(t) for t in ctx.jclean(to_dev(img), to_dev(psfs), "sum", **kw, **dev))
            assert same_bits(r1, r2[0]) and same_bits(m1, m2[0]), auto
            # [iterations, peak, index, flux, T, reason, first peak, 0] against [iterations, s, index, L, reason, s1, 0, 0, flux_0 ..]
            assert same_bits(s1[[0, 1, 2, 3, 4, 5, 6]], s2[[0, 1, 2, 8, 3, 4, 5]]) and not s2[6:8].any() and not s2[9:].any()
            if "noise" in auto and math.isnan(auto["noise"]):
                assert s1[5] == 3 and s1[0] == 0 and np.array_equal(r1, img[0])
            else:
                assert s1[0] > 3 and np.count_nonzero(m1) > 1
    # weights=None through the C ABI itself (the binding always passes an array)
    res, models, stats = to_dev(img), torch.zeros((1, N, N), dtype=torch.float64, device="cuda:0"), to_dev(np.zeros(16))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert ctx._lib.gridhip_jclean_dev(ctx._h, N, 1, 1, p(to_dev(psfs)), p(res), p(models), None, 0, GAIN, 0.0, 50, 0, 0,
                                       None, 0.0, None, 0.0, p(stats)) == 0
    m1, r1, s1 = (host(t) for t in ctx.clean(to_dev(img[0]), to_dev(psfs[0]), gain=GAIN, niter=50, peak_frac=1e-9))
    assert same_bits(host(res)[0], r1) and same_bits(host(models)[0], m1) and host(stats)[0] == s1[0] == 50


# ---- exact fixtures: bit for bit -----------------------------------------------------------------------------------------------
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def want(f):
    out = J.reference(f)
    for a in out:
        a.setflags(write=False)
    return out


def place(arr, o):
    """(buffer, view): a device buffer of sentinels four cells longer than arr, and arr in it from cell o <= 3 on (a plain
    torch allocation is 256-byte aligned, so an odd o is a base 8 bytes off)"""
    import torch
    flat = to_dev(np.ascontiguousarray(arr).ravel())
    buf = torch.full((flat.numel() + 4,), SENTINEL, dtype=flat.dtype, device=flat.device)
    buf[o:o + flat.numel()].copy_(flat)
    return buf, buf[o:o + flat.numel()].view(arr.shape)


def guards_hold(buf, o, n):
    b = host(buf)
    return bool((b[:o] == SENTINEL).all() and (b[o + n:] == SENTINEL).all())


def run_fixture(ctx, f, offs=(0, 0, 0), form="dev"):
    """(models, residuals, stats) of the fixture; device form: residuals, PSFs and models start offs cells into buffers
    of their own whose other cells are sentinels, and the PSFs and the mask are read only"""
    psfs, res = np.array(J.exact_psfs(f.N, f.Q)), J.residuals_of(f)
    kw = J.keywords(f)
    if form == "host":
        m, r, s = ctx.jclean(res, psfs, models=np.zeros_like(res), **kw)
        return m, r, s
    (rb, rv), (pb, pv), (mb, mv) = place(res, offs[0]), place(psfs, offs[1]), place(np.zeros_like(res), offs[2])
    mask = kw.pop("mask")
    dmask = None if mask is None else to_dev(mask)
    m, r, s = ctx.jclean(rv, pv, models=mv, mask=dmask, **kw)
    assert m is mv and r is rv
    out = host(m), host(r), host(s)
    for what, buf, o, n in (("residuals", rb, offs[0], res.size), ("psfs", pb, offs[1], psfs.size), ("models", mb, offs[2], res.size)):
        assert guards_hold(buf, o, n), f"{f.name} offsets {offs}: a cell next to the {what} was written"
    assert np.array_equal(host(pv), psfs), f"{f.name}: the PSFs were written"
    assert mask is None or np.array_equal(host(dmask), mask), f"{f.name}: the mask was written"
    return out


def assert_bits(got, ref, what):
    for name, g, w in zip(("models", "residuals", "stats"), got, ref):
        if not same_bits(g, w):
            g, w = np.asarray(g).ravel(), np.asarray(w, dtype=np.float64).ravel()
            bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError(f"{what}: {name} differs at {len(bad)} cells, first "
                                 f"{[(int(i), g[i], w[i]) for i in bad[:4]]}; stats {got[2]} against {ref[2]}")


def ids(fixtures):
    return dict(argnames="f", argvalues=fixtures, ids=[f.name for f in fixtures])


@pytest.mark.parametrize(**ids(J.size_fixtures()))
def test_small_images_odd_sizes_and_the_rim(ctx, f):
    """N from 1 up, one row or column past a tile, odd N with several planes (their slots are 8 bytes apart in alignment),
    components in the four corners: every update region is clipped"""
    assert_bits(run_fixture(ctx, f), want(f), f.name)


@pytest.mark.parametrize("offs", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)])
@pytest.mark.parametrize(**ids([f for f in J.size_fixtures() if f.N in (5, 128, 129) and f.patch == 0]))
def test_a_base_pointer_8_bytes_off(ctx, f, offs):
    """a view one double into a larger buffer, for the residuals, the PSFs and the models in turn and together"""
    assert_bits(run_fixture(ctx, f, offs), want(f), f"{f.name} {offs}")


@pytest.mark.parametrize(**ids(J.tie_fixtures()))
def test_ties_go_to_the_lowest_flat_index(ctx, f):
    """two cells tied in s whose per-plane values differ: in one slot, two rows of a wave, two tiles, two table entries"""
    assert_bits(run_fixture(ctx, f), want(f), f.name)


@pytest.mark.parametrize(**ids(J.exclusion_fixtures()))
def test_nan_masks_and_stop_levels(ctx, f):
    """a NaN in one plane at the would-be peak, under weight 0 too; all NaN, an all-zero mask: reason 2; a NaN sigma:
    reason 3, nothing but stats touched; a stop level from threshold and nsigma * sigma: reason 1"""
    got = run_fixture(ctx, f)
    assert_bits(got, want(f), f.name)
    if f.name.startswith(("all-nan", "one-plane-nan", "zero-mask")):
        assert got[2][4] == 2 and got[2][2] == -1 and math.isnan(got[2][1])
    if f.name.startswith("nan-sigma"):
        assert got[2][4] == 3 and same_bits(got[1], J.residuals_of(f)) and not got[0].any()


@pytest.mark.parametrize(**ids(J.weight_fixtures()))
def test_a_plane_of_weight_zero_is_cleaned_but_does_not_steer(ctx, f):
    got = run_fixture(ctx, f)
    assert_bits(got, want(f), f.name)
    if f.name.startswith("weights-1000"):
        import torch
        # plane 0's own sequence: gridhip_clean of plane 0 alone leaves the same plane 0
        kw = dict(gain=f.gain, threshold=0.0, niter=f.niter, border=f.border, patch=f.patch)
        m0, r0, _ = ctx.clean(to_dev(J.residuals_of(f)[0]), to_dev(np.array(J.exact_psfs(f.N, f.Q)[0])), **kw)
        torch.cuda.synchronize()
        assert same_bits(host(m0), got[0][0]) and same_bits(host(r0), got[1][0])
        for p in range(1, f.P):
            assert np.array_equal(np.flatnonzero(got[0][p]), np.flatnonzero(got[0][0]))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """every argument rule of the header, before anything is touched: arrays and stats stay as they were"""
    import torch
    import gridhip
    EINVAL = gridhip._lib.EINVAL
    N, P = 16, 4
    full = lambda n, v, dt=torch.float64: torch.full((n,), v, dtype=dt, device="cuda:0")  # noqa: E731
    plane = N * N
    psfs, img, models, stats, noise = full(P * plane, 1.0), full(P * plane, 2.0), full(P * plane, 3.0), full(16, 5.0), full(1, 0.5)
    mask, big = full(plane, 1, torch.uint8), full(3 * P * plane, 4.0)
    lib, h = ctx._lib, ctx._h
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    wts = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    good = dict(N=N, P=P, Q=P, psfs=p(psfs), res=p(img), models=p(models), w=None, metric=1, gain=0.1, threshold=0.0, niter=5,
                border=0, patch=0, mask=p(mask), nsigma=2.0, noise=p(noise), peak_frac=0.1)
    nan, inf, B = float("nan"), float("inf"), 8 * plane
    bad = [dict(N=0), dict(gain=0.0), dict(gain=1.5), dict(gain=nan), dict(threshold=-1.0), dict(threshold=nan), dict(niter=-1),
           dict(border=-1), dict(border=N // 2), dict(patch=-1), dict(nsigma=-1.0), dict(nsigma=nan), dict(nsigma=inf),
           dict(peak_frac=1.0), dict(peak_frac=-0.1), dict(peak_frac=nan), dict(noise=None), dict(psfs=None), dict(res=None),
           dict(models=None),
           dict(P=0), dict(P=9, Q=9), dict(P=-1), dict(Q=2), dict(Q=0), dict(Q=3), dict(metric=2), dict(metric=-1),
           dict(w=wts(1, 1, -1, 1)), dict(w=wts(1, nan, 1, 1)), dict(w=wts(1, inf, 1, 1)), dict(w=wts(0, 0, 0, 0)),
           dict(models=p(img)),                                  # models and residuals are one array
           dict(models=p(img, 3 * B)),                           # the models' first plane is the residuals' last
           dict(psfs=p(big), res=p(big, P * B - 8)),             # the residuals start in the PSFs' last cell
           dict(Q=1, psfs=p(big, B - 8), res=p(big, B - 16), models=p(models)),  # Q = 1: one PSF plane, still overlapped
           dict(psfs=p(big, 2 * P * B - 8), models=p(big, P * B)),  # the PSFs start in the models' last cell
           dict(mask=p(img, (P - 1) * B)),                       # the mask lies in the residuals' last plane
           dict(mask=p(models, B + 1)), dict(mask=p(psfs, P * B - 1))]
    order = ("N", "P", "Q", "psfs", "res", "models", "w", "metric", "gain", "threshold", "niter", "border", "patch", "mask",
             "nsigma", "noise", "peak_frac")
    for form in (lib.gridhip_jclean_dev, lib.gridhip_jclean):
        for b in bad:
            a = dict(good, **b)
            assert form(h, *(a[k] for k in order), p(stats)) == EINVAL, b
    # Q = 1 reads one PSF plane: residuals that start right after it are no overlap
    ok = dict(good, Q=1, psfs=p(big), res=p(big, B), models=p(big, (1 + P) * B), mask=None, nsigma=0.0, noise=None, niter=0)
    assert lib.gridhip_jclean_dev(h, *(ok[k] for k in order), p(stats)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(stats)[:6], [0.0, 64.0, 0.0, 0.1 * 0.1 * 64.0, 0.0, 64.0])  # (niter = 0: s = 4 * 4^2 at cell 0)
    for t, v in ((psfs, 1.0), (img, 2.0), (models, 3.0), (big, 4.0), (noise, 0.5), (mask, 1)):
        assert bool((t == v).all())
    with pytest.raises(gridhip.GridHipError) as ei:  # overlapping models and residuals through the binding
        both = torch.zeros((P + 1, N, N), dtype=torch.float64, device="cuda:0")
        ctx.jclean(both[:P], psfs.view(P, N, N), models=both[1:])
    assert ei.value.code == EINVAL


# ---- forms ------------------------------------------------------------------------------------------------------------------------
def test_host_and_dev_forms_give_the_same_bits(ctx):
    """Host form == _dev form on the same arrays, bit for bit, and twice over; the second call of a shape allocates nothing"""
    import torch
    N, P = 129, 4  # odd, two tile columns
    for Q, metric in ((1, 1), (P, 0)):
        psfs, img = jclean_ref.make_psfs(N, Q), jclean_ref.make_sky(N, P, Q)
        mask = np.random.default_rng(9).random((N, N)) < 0.8
        kw = dict(gain=0.2, threshold=0.0, niter=120, border=3, patch=0, nsigma=1.0, peak_frac=0.01)
        weights = [1.0, 0.5, 0.5, 0.25]
        outs = []
        for rep in range(2):
            a = img.copy()
            m, r, s = ctx.jclean(a, psfs, METRIC[metric], weights, mask=mask, noise=1e-3, **kw)
            assert r is a
            outs.append((m, r, s))
            outs.append(tuple(host(t) for t in ctx.jclean(to_dev(img), to_dev(psfs), METRIC[metric], weights, mask=to_dev(mask),
                                                          noise=to_dev(np.array([1e-3])), **kw)))
        assert outs[0][2][0] > 20 and np.count_nonzero(outs[0][0]) > 8
        for o in outs[1:]:
            for x, y in zip(o, outs[0]):
                assert np.array_equal(x, y)
        # the third and fourth calls of the shape: the pool serves them
        dimg, dpsfs, dmask, dnoise = to_dev(img), to_dev(psfs), to_dev(mask), to_dev(np.array([1e-3]))
        models = torch.zeros((P, N, N), dtype=torch.float64, device="cuda:0")
        ctx.jclean(dimg, dpsfs, METRIC[metric], weights, mask=dmask, noise=dnoise, models=models, **kw)
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()[0]
        st = [ctx.jclean(dimg, dpsfs, METRIC[metric], weights, mask=dmask, noise=dnoise, models=models, **kw)[2] for _ in range(2)]
        torch.cuda.synchronize()
        assert torch.cuda.mem_get_info()[0] == free and ctx.get_option("errors") == 0 and host(st[1])[0] >= 0


def test_jclean_can_be_captured_into_a_hip_graph(ctx):
    """test_gpu_mfclean.py's capture: a warm-up on the capture stream, the capture of one linear chain, two replays on
    changed contents against the eager call"""
    import torch
    N, P, Q = 255, 3, 3
    psfs, img = jclean_ref.make_psfs(N, Q), jclean_ref.make_sky(N, P, Q)
    kw = dict(metric="sumsq", gain=0.2, threshold=0.0, niter=30, border=0, patch=16)
    dpsfs, dirty = to_dev(psfs), to_dev(img)
    res = torch.zeros((P, N, N), dtype=torch.float64, device="cuda:0")
    models = torch.zeros((P, N, N), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream
        ctx.jclean(res, dpsfs, models=models, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, _, st = ctx.jclean(res, dpsfs, models=models, **kw)
    torch.cuda.synchronize()
    for rep in range(2):
        res.copy_(dirty * (rep + 1))
        models.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (models, res, st)]
        em, er, es = ctx.jclean(dirty * (rep + 1), dpsfs, **kw)
        torch.cuda.synchronize()
        assert np.count_nonzero(got[0]) > 0 and got[2][0] == 30
        for a, b in zip(got, (em, er, es)):
            assert np.array_equal(a, host(b))
    assert ctx.get_option("errors") == 0


# ---- the joint major cycle ----------------------------------------------------------------------------------------------------------
def one_visibility_per_cell_imager(ctx, theta, lam, N):
    """(imager, n): a `simple` imager whose n = 20000 baselines fall into 20000 different uv cells, all with v > 0 (nothing
    is mirrored onto another's cell): 100 rows of 200 cells, each visibility up to 0.2 cells off its cell's centre, in a
    shuffled order.  The simple gridder adds every visibility to its cell with a global fp64 atomic, and with several
    visibilities per cell the order of those additions - and so the last bit of a dirty image - changes from one call of
    Imager.cycle to the next (measured on an MI355X with a random stream of this size: 1.2e-16 of the peak between two
    calls on the same arguments).  With one visibility per cell every sum has one term and a major cycle repeats its bits,
    so that two runs of the same calls can be compared bit for bit - which the test asserts of cycle itself first."""
    rng = np.random.default_rng(91)
    ky, kx = np.mgrid[1:101, -100:100]
    order = rng.permutation(ky.size)
    cell = 1.0 / theta  # wavelengths per uv cell
    u = (kx.ravel()[order] + rng.uniform(-0.2, 0.2, ky.size)) * cell
    v = (ky.ravel()[order] + rng.uniform(-0.2, 0.2, ky.size)) * cell
    w = rng.uniform(-100.0, 100.0, ky.size)
    assert np.abs(u).max() < 0.5 * lam and v.max() < 0.5 * lam and v.min() > 0
    im = ctx.imager(theta, lam, tuple(to_dev(x) for x in (u, v, w)), ("simple",))
    assert im.N == N and im.n == ky.size
    return im, ky.size


def test_joint_deconvolve_is_the_loop_it_replaces(ctx):
    """Four Stokes streams of a small polarised point-source sky through one imager: the composition equals the
    hand-written loop of cycle / jclean calls bit for bit, the four models have identical supports - and four independent
    Imager.deconvolve runs do not, which is what the feature is for."""
    import torch
    import gridhip
    theta, lam, N = 0.1, 2560, 256
    im, n = one_visibility_per_cell_imager(ctx, theta, lam, N)
    rng = np.random.default_rng(92)
    sky = np.zeros((4, N, N))
    for _ in range(5):  # I, and Q, U of up to 30 % of it; no V at all: that plane is noise
        y, x, a = rng.integers(N // 4, N - N // 4), rng.integers(N // 4, N - N // 4), rng.uniform(0.5, 1.0)
        sky[0, y, x], sky[1, y, x], sky[2, y, x] = a, 0.3 * a * rng.uniform(-1, 1), 0.3 * a * rng.uniform(-1, 1)
    noise = 0.05 * (rng.normal(size=(4, n)) + 1j * rng.normal(size=(4, n)))
    vis = torch.stack([im.predict(to_dev(sky[p])) for p in range(4)]) + to_dev(noise)
    # precondition: on this stream a major cycle repeats its bits (see one_visibility_per_cell_imager)
    half = to_dev(0.5 * sky[0])
    first = host(im.cycle(vis[0], model=half)).copy()
    assert all(np.array_equal(host(im.cycle(vis[0], model=half)), first) for _ in range(3)), "cycle does not repeat its bits"
    kw = dict(gain=0.2, threshold=0.0, niter=25, border=2, patch=0, nsigma=1.0)
    models, images, stats = gridhip.joint_deconvolve([im] * 4, vis, 2, metric="sumsq", noise_plane=3, **kw)
    # the same, written out
    m2 = torch.zeros((4, N, N), dtype=torch.float64, device="cuda:0")
    i2 = torch.zeros((4, N, N), dtype=torch.float64, device="cuda:0")
    psfs, rows = im.psf.reshape(1, N, N), []
    for cyc in range(2):
        for p in range(4):
            im.cycle(vis[p], model=m2[p], out=i2[p])
        sigma = ctx.image_stats(i2[3], border=2)[3:4]
        rows.append(host(ctx.jclean(i2, psfs, "sumsq", None, models=m2, noise=sigma, **kw)[2]))
    for p in range(4):
        im.cycle(vis[p], model=m2[p], out=i2[p])
    torch.cuda.synchronize()
    gm, gi, gs = host(models), host(images), host(stats)
    assert gs.shape == (2, 16) and gs[0][0] > 3 and np.count_nonzero(gm[0]) > 3
    assert np.array_equal(gs, np.array(rows)) and np.array_equal(gm, host(m2)) and np.array_equal(gi, host(i2))
    support = [np.flatnonzero(gm[p]) for p in range(4)]
    assert all(np.array_equal(support[0], sp) for sp in support[1:]), "one component list for all four planes"
    # plane by plane: every clean picks its own peaks
    alone = [np.flatnonzero(host(im.deconvolve(vis[p], 2, gain=0.2, niter=25, border=2)[0])) for p in range(4)]
    assert not all(np.array_equal(alone[0], sp) for sp in alone[1:])
    assert ctx.get_option("errors") == 0
    im.close()
