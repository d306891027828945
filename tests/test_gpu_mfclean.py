"""The multi-term CLEAN on the device (gridhip_mfclean*, gridhip_imager_mfclean_dev) against the numpy restatement of
include/gridhip.h's definition (tests/mfclean_ref.py).

Tolerance and preconditions are test_gpu_clean.py's: identical iteration counts, final index and component positions;
models, residuals and stats within 1e-10 of the image's peak (nothing is accumulated with atomics: the residuals are
expected bit for bit, the models to the last bit of a fused step; each figure is printed before it is asserted).
Precondition, asserted on the restatement alone: over all iterations the relative gap between the two largest scores
exceeds 1e-8 - with a smaller gap a last-bit difference could legitimately change the component sequence."""
import ctypes as C
import functools

import numpy as np
import pytest

import mfclean_ref
from test_gpu_imager import Case, host, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-10
GAIN = 0.2


@functools.lru_cache(maxsize=None)
def inputs(N, T, seed=0):
    """(psfs, dirty images): shared between the tests, never written to"""
    psfs = mfclean_ref.make_psfs(N, 100 + seed, T)
    img, _ = mfclean_ref.make_sky(psfs, 101 + seed)
    return psfs, img


def run_ref(psfs, img, **kw):
    res, models, trace = img.copy(), np.zeros_like(img), []
    stats = mfclean_ref.mfclean(psfs, res, models, kw["gain"], kw["threshold"], kw["niter"], kw["border"], kw["patch"],
                                trace)
    return models, res, stats, trace


def run_dev(ctx, psfs, img, **kw):
    m, r, s = ctx.mfclean(to_dev(img), to_dev(psfs), **kw)
    return host(m), host(r), host(s)


def compare(got, want, peak, what):
    gm, gr, gs = got
    wm, wr, ws = want[:3]
    assert gs[0] == ws[0], f"{what}: {gs[0]} iterations, the reference {ws[0]}"
    assert gs[2] == ws[2], f"{what}: final peak at {gs[2]}, the reference {ws[2]}"
    assert gs[7] == ws[7], f"{what}: reason {gs[7]}, the reference {ws[7]}"
    assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(wm)), f"{what}: component positions differ"
    errs = (np.abs(gm - wm).max() / peak, np.abs(gr - wr).max() / peak, np.abs(gs - ws)[[1, 3, 4, 5, 6]].max() / peak)
    print(f"{what}: models {errs[0]:.2e} residuals {errs[1]:.2e} stats {errs[2]:.2e}")
    assert max(errs) < TOL, (what, errs)
    return errs


@pytest.mark.parametrize("patch", [0, 32])
@pytest.mark.parametrize("wide_border", [False, True])
# N: even, odd (the planes' slots are misaligned), several tile rows and columns; T = 4, the most terms, at the first two
@pytest.mark.parametrize("N,T", [(N, T) for N in (256, 255, 600) for T in (1, 2, 3)] + [(256, 4), (255, 4)])
def test_against_the_restatement(ctx, N, T, wide_border, patch):
    psfs, img = inputs(N, T)
    peak = np.abs(img[0]).max()
    border = N // 8 if wide_border else 0
    mid = 0.5 * peak if T < 4 else mfclean_ref.midway_threshold(psfs, img, border, patch)
    worst, bits = 0.0, True
    for threshold, midway in ((0.0, False), (mid, True)):
        for niter in (0, 1, 200):
            kw = dict(gain=GAIN, threshold=threshold, niter=niter, border=border, patch=patch)
            want = run_ref(psfs, img, **kw)
            gaps = [g for _, g in want[3]]
            assert not gaps or min(gaps) > 1e-8, f"precondition: smallest gap {min(gaps):.2e} (change the seed)"
            if niter == 200:
                # the two thresholds: one stops the loop midway, the other is never reached
                assert (0 < want[2][0] < niter and want[2][7] == 1) if midway else \
                    (want[2][0] == niter and want[2][7] == 0), want[2]
            got = run_dev(ctx, psfs, img, **kw)
            errs = compare(got, want, peak, f"N {N} T {T} {kw}")
            worst = max(worst, *errs)
            bits = bits and np.array_equal(got[1], want[1])
    print(f"N {N} T {T} border {border} patch {patch}: worst {worst:.2e}, residuals bit for bit {bits}")


@pytest.mark.parametrize("N", [256, 255])
def test_one_term_with_a_normalised_psf_is_clean_bit_for_bit(ctx, N):
    psfs, img = inputs(N, 1)
    assert psfs[0][N // 2, N // 2] == 1.0
    for border, patch in ((0, 0), (N // 8, 32)):
        kw = dict(gain=GAIN, threshold=0.0, niter=150, border=border, patch=patch)
        m1, r1, s1 = (host(t) for t in ctx.clean(to_dev(img[0]), to_dev(psfs[0]), **kw))
        m2, r2, s2 = run_dev(ctx, psfs, img, **kw)
        assert s1[0] == 150 and np.count_nonzero(m1) > 1
        assert np.array_equal(r1, r2[0]) and np.array_equal(m1, m2[0])
        assert np.array_equal(s2, [s1[0], s1[1], s1[2], s1[3], 0.0, 0.0, 0.0, 0.0])


def test_host_dev_and_imager_forms_give_the_same_bits(ctx):
    """Host form == _dev form == Imager.mfclean on the same arrays, bit for bit, and twice over."""
    import torch
    c = Case(ctx, "w_cache", 0.1, 1290, 4000, 31)  # N = 129: odd, two tile columns
    rng = np.random.default_rng(32)
    c.im.set_spectral(to_dev(rng.choice(np.linspace(-0.2, 0.2, 8), c.im.n)), 2)
    psfs = host(c.im.spectral_psfs()).copy()
    img = host(c.im.mfs_cycle(c.dvis)).copy()
    torch.cuda.synchronize()
    kw = dict(gain=0.2, threshold=0.0, niter=120, border=3, patch=0)
    outs = []
    for rep in range(2):
        a = img.copy()
        m, r, s = ctx.mfclean(a, psfs, **kw)
        assert r is a
        outs.append((m, r, s))
        outs.append(tuple(host(t) for t in ctx.mfclean(to_dev(img), to_dev(psfs), **kw)))
        outs.append(tuple(host(t) for t in c.im.mfclean(to_dev(img), **kw)))
    assert outs[0][2][0] == 120 and np.count_nonzero(outs[0][0]) > 2
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert np.array_equal(x, y)
    want = run_ref(psfs, img, **kw)
    assert min(g for _, g in want[3]) > 1e-8
    compare(outs[0], want, np.abs(img[0]).max(), "imager psfs")
    c.im.close()


def test_stopped_early_the_trailing_launches_are_no_ops(ctx):
    N, T = 256, 2
    psfs, img = inputs(N, T, 1)
    peak = np.abs(img[0]).max()
    kw = dict(gain=0.25, threshold=0.8 * peak, niter=300, border=0, patch=0)
    want = run_ref(psfs, img, **kw)
    assert 0 < want[2][0] < 40 and want[2][7] == 1, want[2]
    got = run_dev(ctx, psfs, img, **kw)
    compare(got, want, peak, "stopped early")
    assert np.array_equal(got[1], want[1])  # the residuals are what the restatement leaves, which stops there


def test_models_are_accumulated_and_nan_is_never_selected(ctx):
    import torch
    N, T = 255, 2
    psfs, img = inputs(N, T, 2)
    img = img.copy()
    img[0, 7, 9], img[1, 200, 100] = np.nan, np.nan  # a NaN in either term hides its cell
    kw = dict(gain=0.1, threshold=0.0, niter=60, border=0, patch=40)
    start = np.random.default_rng(5).normal(size=(T, N, N))
    res, models = img.copy(), start.copy()
    ws = mfclean_ref.mfclean(psfs, res, models, kw["gain"], kw["threshold"], kw["niter"], kw["border"], kw["patch"])
    dm = to_dev(start)
    m, r, s = ctx.mfclean(to_dev(img), to_dev(psfs), models=dm, **kw)
    assert m is dm
    gm, gr, gs = host(m), host(r), host(s)
    peak = np.nanmax(np.abs(img[0]))
    assert gs[0] == ws[0] == 60 and gs[2] == ws[2] and gs[7] == ws[7] == 0
    assert gs[2] not in (7 * N + 9, 200 * N + 100)
    assert np.nanmax(np.abs(gr - res)) / peak < TOL and np.array_equal(np.isnan(gr), np.isnan(res))
    assert np.abs(gm - models).max() / peak < TOL and np.abs(gs - ws).max() / peak < TOL
    # every cell NaN: nothing to select, nothing changes
    allnan = torch.full((T, N, N), float("nan"), dtype=torch.float64, device="cuda:0")
    m, r, s = ctx.mfclean(allnan, to_dev(psfs), niter=5)
    gs = host(s)
    assert gs[0] == 0 and np.isnan(gs[1]) and gs[2] == -1 and not gs[3:7].any() and gs[7] == 2 and not host(m).any()


def test_a_singular_hessian_changes_nothing(ctx):
    N = 64
    psfs, img = inputs(N, 2, 3)
    sing = np.stack([psfs[0]] * 3)  # P_1 = P_0, P_2 = P_0: the second pivot is 0
    start = np.full((2, N, N), 3.0)
    m, r, s = run_dev(ctx, sing, img, models=to_dev(start), gain=0.2, threshold=0.0, niter=10, border=0, patch=0)
    assert np.array_equal(r, img) and np.array_equal(m, start)
    assert s[0] == 0 and np.isnan(s[1]) and s[2] == -1 and not s[3:7].any() and s[7] == 3
    assert mfclean_ref.mfclean(sing, img.copy(), start.copy(), 0.2, 0.0, 10)[7] == 3


def test_refusals(ctx):
    """every argument rule of the header, GRIDHIP_EINVAL, before anything is touched"""
    import torch
    import gridhip
    N, T = 16, 2
    psfs = torch.full((3, N, N), 1.0, dtype=torch.float64, device="cuda:0")
    img, models = (torch.full((T, N, N), v, dtype=torch.float64, device="cuda:0") for v in (2.0, 3.0))
    good = dict(gain=0.1, threshold=0.0, niter=5, border=0, patch=0)
    bad = [dict(gain=0.0), dict(gain=1.5), dict(gain=float("nan")), dict(threshold=-1.0), dict(threshold=float("nan")),
           dict(niter=-1), dict(border=-1), dict(border=N // 2), dict(patch=-1)]
    for b in bad:
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.mfclean(img, psfs, models=models, **dict(good, **b))
        assert ei.value.code == gridhip._lib.EINVAL, b
    big = torch.full((8 * N * N,), 4.0, dtype=torch.float64, device="cuda:0")
    lib, h = ctx._lib, ctx._h
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    plane = 8 * N * N
    calls = [(N, 0, p(psfs), p(img), p(models)), (N, 5, p(psfs), p(img), p(models)), (0, T, p(psfs), p(img), p(models)),
             (N, T, None, p(img), p(models)), (N, T, p(psfs), None, p(models)), (N, T, p(psfs), p(img), None),
             (N, T, p(psfs), p(img), p(img)), (N, T, p(psfs), p(psfs), p(models)),
             (N, T, p(psfs), p(img), p(img, plane)),            # models' first plane is the residuals' second
             (N, T, p(big), p(big, 3 * plane - 8), p(models)),  # the residuals overlap the last PSF by one cell
             (N, T, p(big, 2 * plane - 8), p(img), p(big))]     # the PSFs start in the models' last cell
    for form in (lib.gridhip_mfclean_dev, lib.gridhip_mfclean):
        for n_, t_, a, b, c_ in calls:
            assert form(h, n_, t_, a, b, c_, 0.1, 0.0, 5, 0, 0, None) == gridhip._lib.EINVAL
    torch.cuda.synchronize()
    assert bool((psfs == 1.0).all()) and bool((img == 2.0).all()) and bool((models == 3.0).all()) and bool((big == 4.0).all())


def test_mfclean_can_be_captured_into_a_hip_graph(ctx):
    """test_gpu_clean.py's capture: a warm-up on the capture stream, the capture, two replays on changed contents
    against the eager call"""
    import torch
    N, T = 255, 2
    psfs, img = inputs(N, T)
    kw = dict(gain=0.2, threshold=0.0, niter=30, border=0, patch=16)
    dpsfs, dirty = to_dev(psfs), to_dev(img)
    res = torch.zeros((T, N, N), dtype=torch.float64, device="cuda:0")
    models = torch.zeros((T, N, N), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream
        ctx.mfclean(res, dpsfs, models=models, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, _, st = ctx.mfclean(res, dpsfs, models=models, **kw)
    torch.cuda.synchronize()
    for rep in range(2):
        res.copy_(dirty * (rep + 1))
        models.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (models, res, st)]
        em, er, es = ctx.mfclean(dirty * (rep + 1), dpsfs, **kw)
        torch.cuda.synchronize()
        assert np.count_nonzero(got[0]) > 0 and got[2][0] == 30
        for a, b in zip(got, (em, er, es)):
            assert np.array_equal(a, host(b))
    assert ctx.get_option("errors") == 0
