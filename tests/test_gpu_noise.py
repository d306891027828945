"""Image statistics, clean masks and noise-based stop levels on the device (gridhip_image_stats*, gridhip_*clean_auto*,
gridhip_imager_*deconvolve_auto_dev) against the numpy restatements of include/gridhip.h's definitions
(tests/noise_ref.py, tests/clean_auto_ref.py).

image_stats is an order statistic: every comparison is bit for bit.  clean_auto rounds as the restatement does and is
compared bit for bit too.  msclean_auto's set-up convolutions fuse their multiply-adds, which numpy cannot restate
(tests/msclean_ref.py says why), so with more than the delta scale its images are compared as test_gpu_msclean.py
compares them: identical component positions, counts and reasons, values within 1e-10 of the image's peak.  The loops
are compared with the calls they replace within the same 1e-10, the bound test_deconvolve_is_the_loop_it_replaces
allows for the same reason (the cycle's fp64 atomics).
Preconditions, asserted on the reference alone: no peak the stop test looks at lies within 1e-6 relative of T, and the
gap between the two largest cells exceeds 1e-8 - else a last-bit difference could change an iteration count."""
import ctypes as C
import functools

import numpy as np
import pytest

import clean_auto_ref
import clean_ref
import noise_ref
from test_gpu_imager import Case, host, to_dev
from test_gpu_msclean import SCALES
from test_gpu_msclean import fixture as ms_fixture

pytestmark = pytest.mark.gpu
TOL = 1e-10


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- image_stats ----------------------------------------------------------------------------------------------------------
def patterns(N, seed):
    rng = np.random.default_rng(seed)
    n = N * N
    out = {"gaussian": rng.normal(size=n), "equal": np.full(n, 0.3)}
    two = np.where(np.arange(n) % 2 == 0, -1.5, 2.5)
    out["two values"] = two
    mix = rng.choice([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e308, -1e308, 1.7e308, 3.0, -3.0], n)
    out["zeros denormals huge"] = mix
    low = np.full(n, 1.0).view(np.uint64) + rng.integers(0, 7, n).astype(np.uint64)
    out["lowest digit"] = low.view(np.float64)
    bad = rng.normal(size=n)
    bad[rng.integers(0, n, max(1, n // 9))] = np.nan
    bad[rng.integers(0, n, max(1, n // 11))] = np.inf
    bad[rng.integers(0, n, max(1, n // 13))] = -np.inf
    out["nan and inf"] = bad
    return {k: v.reshape(N, N) for k, v in out.items()}


@pytest.mark.parametrize("N", [1, 37, 130, 257, 600])
def test_image_stats_bit_for_bit(ctx, N):
    rng = np.random.default_rng(N)
    for name, img in patterns(N, N).items():
        cases = [(None, 0)]
        if N > 4:
            cases += [(rng.random((N, N)) < 0.4, 0), (None, N // 5), ((rng.random((N, N)) < 0.7).astype(np.uint8) * 3, 2)]
        for mask, border in cases:
            want = noise_ref.image_stats(img, mask, border)
            got = host(ctx.image_stats(to_dev(img), None if mask is None else to_dev(mask), border))
            assert same(got, want), f"N {N} {name} mask {mask is not None} border {border}: {got} != {want}"
    # n even and n odd of two values; masks that leave 0, 1 and 2 cells
    if N > 4:
        img = patterns(N, 1)["two values"]
        for left in (0, 1, 2, N * N - 2 + (N * N) % 2, N * N - 1 - (N * N) % 2):  # ... a large odd and a large even count
            mask = np.zeros(N * N, dtype=bool)
            mask[rng.permutation(N * N)[:left]] = True
            mask = mask.reshape(N, N)
            want = noise_ref.image_stats(img, mask)
            got = host(ctx.image_stats(to_dev(img), to_dev(mask)))
            assert want[0] == left and same(got, want), (N, left, got, want)


def test_image_stats_host_dev_and_imager_forms_twice(ctx):
    c = Case(ctx, "simple", 0.1, 1290, 2000, 5)  # N = 129
    N = c.N
    img = host(c.cycle(c.dvis)).copy()
    img[3, 7] = np.nan
    mask = np.random.default_rng(3).random((N, N)) < 0.8
    want = noise_ref.image_stats(img, mask, 2)
    for rep in range(2):
        outs = [ctx.image_stats(img, mask, 2), host(ctx.image_stats(to_dev(img), to_dev(mask), 2)),
                host(c.im.image_stats(to_dev(img), to_dev(mask), 2))]
        for o in outs:
            assert same(o, want), (o, want)
    ctx.set_option("noise_bits", 8)  # the 8-bit digit gives the same order statistic
    try:
        assert same(host(ctx.image_stats(to_dev(img), to_dev(mask), 2)), want)
    finally:
        ctx.set_option("noise_bits", 0)
    c.im.close()


@pytest.mark.parametrize("N", [37, 257])
def test_image_stats_with_the_8_bit_digit(ctx, N):
    """The public option noise_bits = 8 (8 + 8 passes of equal width) on every value pattern - among them the keys that
    share their high digits and the values that differ in the lowest digit only - with and without a mask and a border."""
    rng = np.random.default_rng(N + 1)
    ctx.set_option("noise_bits", 8)
    try:
        for name, img in patterns(N, N + 1).items():
            for mask, border in ((None, 0), (rng.random((N, N)) < 0.5, 3)):
                want = noise_ref.image_stats(img, mask, border)
                got = host(ctx.image_stats(to_dev(img), None if mask is None else to_dev(mask), border))
                assert same(got, want), f"N {N} {name} mask {mask is not None} border {border}: {got} != {want}"
    finally:
        ctx.set_option("noise_bits", 0)


# ---- clean_auto -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N):
    psf = clean_ref.make_psf(N, 100)
    img, _ = clean_ref.make_sky(psf, 200)
    return psf, img


@functools.lru_cache(maxsize=None)
def ms_setup(N):
    """the restatement's set-up of inputs(N)'s PSF for SCALES - computed once per shape and never changed"""
    import msclean_ref
    return msclean_ref.setup(inputs(N)[0], list(SCALES))


def masks(N):
    rng = np.random.default_rng(N)
    straddle = np.zeros((N, N), dtype=np.uint8)
    x = 127 if N > 130 else N // 2 - 1  # rows 15 / 16 straddle two tile rows; columns 127 / 128 two tile columns at N = 200
    straddle[15:17, x:x + 2] = 1
    return {"random": rng.random((N, N)) < 0.5, "straddle": straddle, "empty": np.zeros((N, N), dtype=bool)}


def margin_ok(trace, T):
    return all(abs(p - T) > 1e-6 * T for _, p, _ in trace) and all(g > 1e-8 for _, _, g in trace[:-1])


@pytest.mark.parametrize("N", [96, 97, 200])
def test_clean_auto_bit_for_bit(ctx, N):
    psf, img = inputs(N)
    peak = np.abs(img).max()
    terms = {"threshold": dict(threshold=0.3 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.05),
             "nsigma": dict(threshold=0.01 * peak, nsigma=3.0, sigma=0.1 * peak, peak_frac=0.05),
             "peak_frac": dict(threshold=0.01 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.3),
             "nan sigma": dict(threshold=0.0, nsigma=3.0, sigma=np.nan, peak_frac=0.0)}
    for mname, mask in masks(N).items():
        for tname, t in terms.items():
            for patch in (0, 20):
                res, model, trace = img.copy(), np.zeros_like(img), []
                ws = clean_auto_ref.clean(psf, res, model, 0.2, t["threshold"], 300, 2, patch, mask, t["nsigma"], t["sigma"],
                                          t["peak_frac"], trace)
                what = f"N {N} mask {mname} term {tname} patch {patch}"
                if tname == "nan sigma":
                    assert ws[5] == 3 and ws[0] == 0
                elif mname == "empty":
                    assert ws[5] == 2 and ws[0] == 0
                else:
                    assert margin_ok(trace, ws[4]), f"precondition, {what}"
                    if mname == "random":
                        assert ws[5] == 1 and ws[0] > 0, (what, ws)
                        assert ws[4] == {"threshold": t["threshold"], "nsigma": t["nsigma"] * t["sigma"],
                                         "peak_frac": t["peak_frac"] * abs(ws[6])}[tname], (what, ws)
                m, r, s = ctx.clean(to_dev(img), to_dev(psf), 0.2, t["threshold"], 300, 2, patch, mask=to_dev(mask),
                                    nsigma=t["nsigma"], noise=to_dev(np.array([t["sigma"]])), peak_frac=t["peak_frac"])
                gm, gr, gs = host(m), host(r), host(s)
                assert same(gs, ws), f"{what}: stats {gs} != {ws}"
                assert same(gr, res) and same(gm, model), what
                assert not gm[np.asarray(mask) == 0].any(), f"{what}: a component outside the mask"
                if ws[5] in (2, 3):
                    assert np.array_equal(gr, img) and not gm.any()
    # the host form gives the same bits
    mask, t = masks(N)["random"], terms["nsigma"]
    a = img.copy()
    m, r, s = ctx.clean(a, psf, 0.2, t["threshold"], 300, 2, 0, mask=mask, nsigma=t["nsigma"], noise=t["sigma"],
                        peak_frac=t["peak_frac"])
    dm, dr, ds = ctx.clean(to_dev(img), to_dev(psf), 0.2, t["threshold"], 300, 2, 0, mask=to_dev(mask), nsigma=t["nsigma"],
                           noise=t["sigma"], peak_frac=t["peak_frac"])
    assert r is a and same(m, host(dm)) and same(r, host(dr)) and same(s, host(ds))


@pytest.mark.parametrize("N", [96, 97, 200])
def test_msclean_auto_against_the_restatement(ctx, N):
    psf, img, pre = ms_fixture(N)
    peak = np.abs(img).max()
    bias = [1.0, 0.76, 0.4]
    terms = {"threshold": dict(threshold=0.3 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.05),
             "nsigma": dict(threshold=0.01 * peak, nsigma=3.0, sigma=0.1 * peak, peak_frac=0.05),
             "peak_frac": dict(threshold=0.01 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.3),
             "nan sigma": dict(threshold=0.0, nsigma=3.0, sigma=np.nan, peak_frac=0.0)}
    for mname, mask in masks(N).items():
        for tname, t in terms.items():
            res, model, trace = img.copy(), np.zeros_like(img), []
            ws = clean_auto_ref.msclean(psf, res, model, SCALES, bias, 0.2, t["threshold"], 40, 2, 0, mask, t["nsigma"],
                                        t["sigma"], t["peak_frac"], trace, pre)
            what = f"N {N} mask {mname} term {tname}"
            if tname == "nan sigma":
                assert ws[13] == 3 and ws[0] == 0
            elif mname == "empty":
                assert ws[13] == 2 and ws[0] == 0
            else:
                assert all(abs(p - ws[12]) > 1e-6 * ws[12] for _, _, p in trace), f"precondition, {what}"
                # no component CENTRE outside the mask, from the restatement's trace
                assert all(np.asarray(mask).flat[k] != 0 for s_, k, _ in trace if s_ >= 0), what
            m, r, s = ctx.msclean(to_dev(np.array(img)), to_dev(np.array(psf)), SCALES, bias, 0.2, t["threshold"], 40, 2, 0,
                                  mask=to_dev(mask), nsigma=t["nsigma"], noise=to_dev(np.array([t["sigma"]])),
                                  peak_frac=t["peak_frac"])
            gm, gr, gs = host(m), host(r), host(s)
            assert np.array_equal(gs[[0, 2, 3, 13]], ws[[0, 2, 3, 13]]) and np.array_equal(gs[5:12], ws[5:12]), (what, gs, ws)
            assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(model)), f"{what}: component positions differ"
            errs = (np.abs(gm - model).max(), np.abs(gr - res).max(), np.nanmax(np.abs(gs - ws)[[1, 4, 12, 14]], initial=0.0))
            print(f"{what}: model {errs[0] / peak:.2e} residual {errs[1] / peak:.2e} stats {errs[2] / peak:.2e}")
            assert max(errs) / peak < TOL and np.isnan(gs[12]) == np.isnan(ws[12]), (what, errs)
            if ws[13] in (2, 3):
                assert np.array_equal(gr, img) and not gm.any()


@pytest.mark.parametrize("N", [97, 200])
def test_masked_msclean_auto_bit_for_bit_where_only_the_delta_is_taken(ctx, N):
    """Where every component is a delta nothing that reaches the caller passes through a set-up convolution - R_0 loses
    f * psf itself and the model one cell - so the restatement gives the bits: model, residual and all 16 stats, for the
    delta scale alone and for the three scales with biases that leave only the delta selectable (the masked tile kernel
    then runs its three slices and the pick kernel reduces three tables), under the random and the straddling mask and
    with each term of T the binding one.  The sky is clean_auto's point sources, so that the loops end by |peak| <= T."""
    psf, img = inputs(N)
    pre = ms_setup(N)
    peak = np.abs(img).max()
    terms = {"threshold": dict(threshold=0.3 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.05),
             "nsigma": dict(threshold=0.01 * peak, nsigma=3.0, sigma=0.1 * peak, peak_frac=0.05),
             "peak_frac": dict(threshold=0.01 * peak, nsigma=1.0, sigma=0.01 * peak, peak_frac=0.3)}
    dpsf = to_dev(np.array(psf))
    for scales, bias, setup in (([0.0], [1.0], None), (SCALES, [1.0, 1e-200, 1e-200], pre)):
        for mname, mask in masks(N).items():
            if mname == "empty":
                continue
            taken = 0
            for tname, t in terms.items():
                res, model, trace = img.copy(), np.zeros_like(img), []
                ws = clean_auto_ref.msclean(psf, res, model, scales, bias, 0.2, t["threshold"], 300, 2, 0, mask, t["nsigma"],
                                            t["sigma"], t["peak_frac"], trace, setup)
                what = f"N {N} scales {scales} mask {mname} term {tname}"
                assert all(abs(p - ws[12]) > 1e-6 * ws[12] for _, _, p in trace), f"precondition, {what}"
                assert ws[6] == ws[0] and all(s_ <= 0 for s_, _, _ in trace), f"precondition: a wide scale taken, {what}"
                taken += ws[0]
                if mname == "random":
                    assert ws[13] == 1 and ws[0] > 0, (what, ws)
                m, r, s = ctx.msclean(to_dev(np.array(img)), dpsf, scales, bias, 0.2, t["threshold"], 300, 2, 0,
                                      mask=to_dev(mask), nsigma=t["nsigma"], noise=to_dev(np.array([t["sigma"]])),
                                      peak_frac=t["peak_frac"])
                gm, gr, gs = host(m), host(r), host(s)
                assert same(gs, ws), f"{what}: stats {gs} != {ws}"
                assert same(gr, res) and same(gm, model), what
                assert not gm[np.asarray(mask) == 0].any(), f"{what}: a component outside the mask"
            assert taken > 0, f"N {N} scales {scales} mask {mname}: no component in any case"


def test_masked_msclean_auto_host_dev_and_imager_forms_give_the_same_bits(ctx):
    """Host form == _dev form == Imager.msclean for a masked multi-scale call with a noise-based stop level, bit for
    bit and twice over, all 16 stats included."""
    c = Case(ctx, "w_cache", 0.1, 1290, 4000, 31)  # N = 129: odd, two tile columns
    N = c.N
    psf = host(c.im.psf).copy()
    img = host(c.cycle(c.dvis))
    mask = np.random.default_rng(6).random((N, N)) < 0.6
    sigma = float(noise_ref.image_stats(img, None, 3)[3])
    kw = dict(gain=0.2, threshold=0.0, niter=80, border=3, patch=0, nsigma=1.0, peak_frac=0.02)
    outs = []
    for rep in range(2):
        a = img.copy()
        m, r, s = ctx.msclean(a, psf, SCALES, mask=mask, noise=sigma, **kw)
        assert r is a
        outs.append((m, r, s))
        dn = to_dev(np.array([sigma]))
        outs.append(tuple(host(t) for t in ctx.msclean(to_dev(img), to_dev(psf), SCALES, mask=to_dev(mask), noise=dn, **kw)))
        outs.append(tuple(host(t) for t in c.im.msclean(to_dev(img), SCALES, mask=to_dev(mask), noise=dn, **kw)))
    st = outs[0][2]
    assert st.shape == (16,) and st[0] > 1 and np.count_nonzero(st[6:12]) >= 2 and st[12] == max(sigma, 0.02 * abs(st[14])), st
    assert not outs[0][0][~mask & (np.abs(outs[0][0]) > 0)].size or np.count_nonzero(st[7:12]) > 0
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert same(x, y)
    c.im.close()


@pytest.mark.parametrize("N", [97, 200])
def test_neutral_arguments_give_the_plain_forms_bits(ctx, N):
    import gridhip
    psf, img = inputs(N)
    kw = dict(gain=0.2, threshold=0.05 * np.abs(img).max(), niter=50, border=1, patch=0)
    plain = [host(t) for t in ctx.clean(to_dev(img), to_dev(psf), **kw)]
    lib, h = ctx._lib, ctx._h
    res, model, stats = to_dev(img), to_dev(np.zeros_like(img)), to_dev(np.zeros(8))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx._use_torch_stream()
    assert lib.gridhip_clean_auto_dev(h, N, p(to_dev(psf)), p(res), p(model), 0.2, kw["threshold"], 50, 1, 0, None, 0.0, None,
                                      0.0, p(stats)) == gridhip._lib.OK
    assert same(host(model), plain[0]) and same(host(res), plain[1]) and same(host(stats)[:4], plain[2])
    assert host(stats)[4] == kw["threshold"]
    mpsf, mimg, _ = ms_fixture(N)
    plain = [host(t) for t in ctx.msclean(to_dev(np.array(mimg)), to_dev(np.array(mpsf)), SCALES, **kw)]
    res, model, stats = to_dev(np.array(mimg)), to_dev(np.zeros_like(mimg)), to_dev(np.zeros(16))
    sc = (C.c_double * 3)(*SCALES)
    bs = (C.c_double * 3)(*(1.0 - 0.6 * np.array(SCALES) / max(SCALES)))
    assert lib.gridhip_msclean_auto_dev(h, N, p(to_dev(np.array(mpsf))), p(res), p(model), 3, sc, bs, 0.2, kw["threshold"], 50,
                                        1, 0, None, 0.0, None, 0.0, p(stats)) == gridhip._lib.OK
    assert same(host(model), plain[0]) and same(host(res), plain[1]) and same(host(stats)[:12], plain[2])


# ---- the loop -----------------------------------------------------------------------------------------------------------------
class AwCase:
    """an aw imager whose kernels are positive bumps, as gridding kernels are, so that its PSF peaks at the centre
    (test_gpu_clean.py::test_an_imagers_psf_peaks_at_the_centre says why), and unit noise visibilities"""

    def __init__(self, ctx, theta, lam, n, seed, A=4):
        from oracle import gridref_np as P
        from test_gpu_clean import bump
        from test_gpu_imager import stream
        self.N = P.haskell_round(theta * lam)
        u, v, w, vis = stream(n, lam, 100.0, seed, span=0.3)
        rng = np.random.default_rng(seed + 1)
        imgfn = ("aw", to_dev(np.broadcast_to(bump(9), (3, 2, 2, 9, 9))), to_dev(np.linspace(-100.0, 100.0, 3)),
                 to_dev(np.broadcast_to(bump(9), (A, 9, 9))))
        self.im = ctx.imager(theta, lam, tuple(to_dev(x) for x in (u, v, w)), imgfn, a1=to_dev(rng.integers(0, A, n)),
                             a2=to_dev(rng.integers(0, A, n)))
        self.dvis = to_dev(vis)


def noisy_sky(c, seed, nsrc=4, amp=3.0):
    """visibilities of a few point sources predicted through the imager, plus the case's own unit noise scaled down"""
    import torch
    N = c.N
    rng = np.random.default_rng(seed)
    sky = np.zeros((N, N))
    for _ in range(nsrc):
        sky[rng.integers(N // 4, N - N // 4), rng.integers(N // 4, N - N // 4)] = rng.uniform(0.5, 1.0)
    vis = c.im.predict(to_dev(sky)) + amp * c.dvis
    torch.cuda.synchronize()
    return vis, sky


@pytest.mark.parametrize("kind,scales", [("simple", None), ("aw", None), ("simple", [0.0, 3.0])])
def test_deconvolve_auto_is_the_loop_it_replaces(ctx, kind, scales):
    import torch
    c = AwCase(ctx, 0.1, 640, 6000, 71) if kind == "aw" else Case(ctx, kind, 0.1, 640, 6000, 71)
    im, N = c.im, c.N
    # (the aw imager's PSF is broad, and the wide scale leaves the plain residual's peak for last: more iterations there,
    # so that a cycle reaches 3 sigma before niter)
    vis, _ = noisy_sky(c, 72, amp=10.0 if kind == "aw" else 3.0)
    mask = np.random.default_rng(9).random((N, N)) < 0.9
    niter = 40 if kind == "simple" and scales is None else 200
    kw = dict(gain=0.3, threshold=0.0, niter=niter, border=2, patch=0)
    extra = {} if scales is None else dict(scales=scales)
    model, image, stats, istats = im.deconvolve(vis, 3, mask=to_dev(mask), nsigma=3.0, peak_frac=0.05, **kw, **extra)
    m2 = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    rows, irows, reasons = [], [], []
    psf = host(im.psf)
    for cyc in range(3):
        img = im.cycle(vis, m2)
        ist = im.image_stats(img, None, kw["border"])
        himg = host(img).copy()
        assert same(host(ist), noise_ref.image_stats(himg, None, kw["border"]))
        # the reference's trace of this minor cycle: nothing the stop test looks at is close to T
        sigma = float(host(ist)[3])
        trace = []
        if scales is None:
            ws = clean_auto_ref.clean(psf, himg.copy(), host(m2).copy(), kw["gain"], 0.0, niter, 2, 0, mask, 3.0, sigma, 0.05, trace)
            T, reason, looked = ws[4], ws[5], [p for _, p, _ in trace]
            _, _, s = im.clean(img, m2, mask=to_dev(mask), nsigma=3.0, noise=ist[3:4], peak_frac=0.05, **kw)
        else:
            ws = clean_auto_ref.msclean(psf, himg.copy(), host(m2).copy(), scales, [1.0, 0.4], kw["gain"], 0.0, niter, 2, 0, mask,
                                        3.0, sigma, 0.05, trace)
            T, reason, looked = ws[12], ws[13], [p for _, _, p in trace]
            _, _, s = im.msclean(img, scales, model=m2, mask=to_dev(mask), nsigma=3.0, noise=ist[3:4], peak_frac=0.05, **kw)
        assert all(abs(p - T) > 1e-6 * T for p in looked), f"precondition: a peak within 1e-6 of T in cycle {cyc}"
        reasons.append(reason)
        rows.append(host(s))
        irows.append(host(ist))
        assert rows[-1][0] == ws[0] and rows[-1][-3] == reason, (cyc, rows[-1], ws)
    assert 1.0 in reasons, f"no major cycle stops by the noise rule: {reasons}"
    closing = host(im.cycle(vis, m2))
    gm, gi, gs, gis = host(model), host(image), host(stats), host(istats)
    mp, ip = np.abs(host(m2)).max(), np.abs(closing).max()
    em, ei = np.abs(gm - host(m2)).max() / mp, np.abs(gi - closing).max() / ip
    print(f"{kind} {scales}: model {em:.2e} image {ei:.2e} reasons {reasons} iterations {[r[0] for r in rows]}")
    assert mp > 0 and em < TOL and ei < TOL
    rows, irows = np.array(rows), np.array(irows)
    assert gs.shape == rows.shape and gis.shape == (3, 8)
    assert np.array_equal(gs[:, 0], rows[:, 0]) and np.array_equal(gs[:, -3], rows[:, -3])
    assert np.array_equal(gis[:, [0, 6]], irows[:, [0, 6]])
    scale = np.abs(irows[:, 5]).max()
    assert np.abs(gs - rows).max() / scale < TOL and np.abs(gis[:, 1:6] - irows[:, 1:6]).max() / scale < TOL
    assert not gm[~mask].any() or scales is not None
    im.close()


# ---- it does its job -----------------------------------------------------------------------------------------------------------
def test_it_does_its_job(ctx):
    """Five point sources through a compact PSF plus white noise of sigma 0.01: image_stats finds sigma within 10 % (on the
    reference too: the sources cover few cells), and a clean under a mask around the sources at 3 sigma leaves no model
    outside the mask and a masked peak of at most T."""
    N, sigma = 200, 0.01
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:N, 0:N]
    psf = np.exp(-0.5 * ((yy - N // 2) ** 2 + (xx - N // 2) ** 2) / 1.5 ** 2)
    img, mask = sigma * rng.normal(size=(N, N)), np.zeros((N, N), dtype=bool)
    for _ in range(5):
        y, x, a = rng.integers(30, N - 30), rng.integers(30, N - 30), rng.uniform(0.5, 1.0)
        img += a * np.roll(np.roll(psf, y - N // 2, 0), x - N // 2, 1)
        mask[y - 5:y + 6, x - 5:x + 6] = True
    ref = noise_ref.image_stats(img)
    assert abs(ref[3] - sigma) < 0.1 * sigma, ref
    dimg = to_dev(img)
    ist = ctx.image_stats(dimg)
    assert same(host(ist), ref)
    m, r, s = ctx.clean(dimg, to_dev(psf), gain=0.2, niter=400, mask=to_dev(mask), nsigma=3.0, noise=ist[3:4])
    gm, gr, gs = host(m), host(r), host(s)
    print(f"sigma {ref[3]:.5f} (injected {sigma}); {gs[0]:.0f} components, masked peak {gs[1]:.4f}, T {gs[4]:.4f}")
    assert gs[5] == 1 and gs[4] == 3.0 * ref[3] and 0 < gs[0] < 400
    assert not gm[~mask].any() and gm.any()
    assert np.abs(gr[mask]).max() <= gs[4] and abs(gs[1]) == np.abs(gr[mask]).max()


# ---- capture -----------------------------------------------------------------------------------------------------------------
def test_stats_clean_auto_and_deconvolve_auto_in_one_graph(ctx):
    import torch
    c = Case(ctx, "w_cache", 0.1, 640, 6000, 81)
    im, N = c.im, c.N
    vis, _ = noisy_sky(c, 82)
    mask = to_dev(np.random.default_rng(2).random((N, N)) < 0.9)
    kw = dict(gain=0.2, threshold=0.0, niter=30, border=0, patch=16)
    auto = dict(mask=mask, nsigma=3.0, peak_frac=0.05)
    dirty = im.cycle(vis).clone()
    img, model, dimg, dmodel = (torch.zeros((N, N), dtype=torch.float64, device="cuda:0") for _ in range(4))

    def work():
        ist = im.image_stats(img, mask)
        _, _, st = im.clean(img, model, noise=ist[3:4], **auto, **kw)
        _, _, dst, dist = im.deconvolve(vis, 2, model=dmodel, out=dimg, **auto, **kw)
        return ist, st, dst, dist
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream: the first calls' allocations
        img.copy_(dirty)
        work()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = work()
    torch.cuda.synchronize()
    for rep in range(2):
        img.copy_(dirty * (rep + 1))
        for t in (model, dmodel, dimg):
            t.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (model, img, *outs, dmodel, dimg)]
        e_img = dirty * (rep + 1)
        e_ist = im.image_stats(e_img, mask)
        em, er, es = im.clean(e_img, None, noise=e_ist[3:4], **auto, **kw)
        dm, di, ds, dis = im.deconvolve(vis, 2, **auto, **kw)
        torch.cuda.synchronize()
        assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[6]) > 0
        for a, b in zip(got[:4], (em, er, e_ist, es)):
            assert same(a, host(b))
        peak = np.abs(host(dirty)).max()
        for a, b in zip(got[4:], (ds, dis, dm, di)):
            assert np.array_equal(a.shape, host(b).shape) and np.abs(a - host(b)).max() / peak < TOL
    assert ctx.get_option("errors") == 0
    im.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import torch
    import gridhip
    EINVAL = gridhip._lib.EINVAL
    N = 16
    psf, img, model = (torch.full((N, N), v, dtype=torch.float64, device="cuda:0") for v in (1.0, 2.0, 3.0))
    mask = torch.ones((N, N), dtype=torch.uint8, device="cuda:0")
    stats = torch.full((16,), 7.0, dtype=torch.float64, device="cuda:0")
    noise = torch.full((1,), 0.5, dtype=torch.float64, device="cuda:0")
    lib, h = ctx._lib, ctx._h
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    ctx._use_torch_stream()
    cl = (0.1, 0.0, 5, 0, 0)
    sc, bs = (C.c_double * 2)(0.0, 2.0), (C.c_double * 2)(1.0, 0.5)
    autos = [(p(mask), -1.0, p(noise), 0.0), (p(mask), float("inf"), p(noise), 0.0), (p(mask), float("nan"), p(noise), 0.0),
             (p(mask), 0.0, p(noise), 1.0), (p(mask), 0.0, p(noise), -0.1), (p(mask), 0.0, p(noise), float("nan")),
             (p(mask), 3.0, None, 0.0), (p(img), 0.0, None, 0.0), (p(model, N * N * 8 - 1), 0.0, None, 0.0)]
    for form in (lib.gridhip_clean_auto_dev, lib.gridhip_clean_auto):
        for a in autos:
            assert form(h, N, p(psf), p(img), p(model), *cl, *a, p(stats)) == EINVAL, a
        assert form(h, N, p(psf), p(img), p(model), 0.0, 0.0, 5, 0, 0, p(mask), 0.0, None, 0.0, p(stats)) == EINVAL  # clean's
    for form in (lib.gridhip_msclean_auto_dev, lib.gridhip_msclean_auto):
        for a in autos:
            assert form(h, N, p(psf), p(img), p(model), 2, sc, bs, *cl, *a, p(stats)) == EINVAL, a
    big = torch.full((N * N + 8,), 4.0, dtype=torch.float64, device="cuda:0")
    calls = [(0, p(img), p(mask), 0, p(stats)), (N, None, p(mask), 0, p(stats)), (N, p(img), p(mask), 0, None),
             (N, p(img), p(mask), -1, p(stats)), (N, p(img), p(mask), N // 2, p(stats)), (N, p(img), p(img), 0, p(stats)),
             (N, p(big), p(mask), 0, p(big, 8 * (N * N - 1))), (N, p(img), p(big), 0, p(big, 8))]
    for form in (lib.gridhip_image_stats_dev, lib.gridhip_image_stats):
        for a in calls:
            assert form(h, *a) == EINVAL, a
        assert form(h, 16 * 65535 + 1, p(img), None, 0, p(stats)) == gridhip._lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((psf == 1.0).all()) and bool((img == 2.0).all()) and bool((model == 3.0).all()) and bool((big == 4.0).all())
    assert bool((mask == 1).all()) and bool((stats == 7.0).all())
    c = Case(ctx, "simple", 0.1, 160, 500, 3)
    im16 = c.im
    for a in autos[:7]:
        assert lib.gridhip_imager_clean_auto_dev(im16._h, p(img), p(model), *cl, *a, p(stats)) == EINVAL
    for a in autos[:6]:
        assert lib.gridhip_imager_deconvolve_auto_dev(im16._h, p(c.dvis), p(model), p(img), 2, *cl, a[0], a[1], a[3], p(stats),
                                                      None) == EINVAL
    assert lib.gridhip_imager_image_stats_dev(im16._h, p(img), p(img), 0, p(stats)) == EINVAL
    torch.cuda.synchronize()
    assert bool((img == 2.0).all()) and bool((model == 3.0).all()) and bool((stats == 7.0).all())
    im16.close()
