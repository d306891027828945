"""Multi-scale CLEAN on the device (gridhip_msclean*, gridhip_imager_msclean_dev, gridhip_imager_msdeconvolve_dev) against
the numpy restatement of include/gridhip.h's definition (tests/msclean_ref.py).

Tolerance: identical iteration counts, final peak positions, per-scale component counts and component positions; model,
residual and stats within 1e-10 of the image's peak, the bound the project uses everywhere (each figure is printed
before it is asserted).  The restatement cannot fuse the multiply-adds of the set-up convolutions, so the two sides'
cross-PSFs differ by rounding (a few 1e-16 of their magnitude).  Precondition, asserted on the reference alone: over all
iterations the relative gap between the two largest |b_s (R_s / q_s)| over all searched cells of all scales exceeds 1e-8 -
with a smaller gap a last-bit difference could legitimately change the component sequence.

The device keeps no trace, so the component SEQUENCE is checked through runs of 1, 2, 3 ... iterations: the scale of the
last component, the flux and the counts after each prefix are the reference trace's."""
import ctypes as C
import functools

import numpy as np
import pytest

import clean_ref
import msclean_ref
import restore_ref
from test_gpu_clean import point_sky
from test_gpu_imager import Case, host, stream
from test_gpu_imager import to_dev as _to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-10
SCALES = [0.0, 4.0, 10.0]
NITER = 150


def to_dev(x):
    """a device copy (the fixtures are read-only arrays, which torch will not wrap)"""
    return _to_dev(np.array(x))


def fixture(N, scales=SCALES, seed=0):
    """(psf, dirty image, setup of the reference) - computed once per shape and never changed"""
    return _fixture(N, tuple(scales), seed)


@functools.lru_cache(maxsize=None)
def _fixture(N, scales, seed):
    psf = restore_ref.smooth_psf(N, 300 + seed, 0.5)
    img, _ = msclean_ref.extended_sky(psf, 400 + seed)
    pre = msclean_ref.setup(psf, list(scales))
    for a in (psf, img):
        a.setflags(write=False)
    return psf, img, pre


def run_ref(N, scales=SCALES, bias=None, seed=0, img=None, start=None, **kw):
    psf, dirty, pre = fixture(N, scales, seed)
    res = (dirty if img is None else img).copy()
    model = np.zeros_like(res) if start is None else start.copy()
    trace = []
    bias = msclean_ref.default_bias(scales) if bias is None else bias
    stats = msclean_ref.msclean(psf, res, model, list(scales), bias, kw["gain"], kw["threshold"], kw["niter"],
                                kw["border"], kw["patch"], trace=trace, pre=pre)
    return model, res, stats, trace


def run_dev(ctx, N, scales=SCALES, bias=None, seed=0, img=None, **kw):
    psf, dirty, _ = fixture(N, scales, seed)
    m, r, s = ctx.msclean(to_dev(dirty if img is None else img), to_dev(psf), scales, bias, **kw)
    return host(m), host(r), host(s)


def compare(got, want, peak, what):
    gm, gr, gs = got
    wm, wr, ws = want[:3]
    assert gs[0] == ws[0], f"{what}: {gs[0]} iterations, the reference {ws[0]}"
    assert gs[2] == ws[2], f"{what}: final peak at {gs[2]}, the reference {ws[2]}"
    assert gs[3] == ws[3] and np.array_equal(gs[5:], ws[5:]), f"{what}: components per scale {gs[3:]}, the reference {ws[3:]}"
    assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(wm)), f"{what}: component positions differ"
    errs = (np.abs(gm - wm).max() / peak, np.nanmax(np.abs(gr - wr)) / peak, np.abs(gs - ws)[[1, 4]].max() / peak)
    print(f"{what}: model {errs[0]:.2e} residual {errs[1]:.2e} stats {errs[2]:.2e}")
    assert max(errs) < TOL, (what, errs)
    return errs


def min_gap(trace):
    return min((g for _, _, g in trace), default=1.0)


@pytest.mark.parametrize("gain", [0.1, 0.25])
@pytest.mark.parametrize("N", [96, 97, 200])
def test_against_the_restatement(ctx, N, gain):
    psf, img, _ = fixture(N)
    peak = np.abs(img).max()
    worst, scales_used = 0.0, set()
    for border in (0, N // 8):
        for patch in (0, 20):
            for threshold, midway in ((0.0, False), (0.3 * peak, True)):
                for niter in (0, 1, NITER):
                    kw = dict(gain=gain, threshold=threshold, niter=niter, border=border, patch=patch)
                    want = run_ref(N, **kw)
                    assert min_gap(want[3]) > 1e-8, f"precondition: smallest gap {min_gap(want[3]):.2e} (change the seed)"
                    if niter == NITER:
                        # the two thresholds: one stops the loop midway, the other is never reached
                        assert (0 < want[2][0] < niter) if midway else want[2][0] == niter, want[2]
                        scales_used |= {s for s, _, _ in want[3]}
                    got = run_dev(ctx, N, **kw)
                    worst = max(worst, *compare(got, want, peak, f"N {N} gain {gain} {kw}"))
    assert len(scales_used) >= 2, scales_used
    print(f"N {N} gain {gain}: worst {worst:.2e}, scales used {sorted(scales_used)}")


@pytest.mark.parametrize("N", [96, 200])
def test_the_component_sequence_prefix_by_prefix(ctx, N):
    kw = dict(gain=0.25, threshold=0.0, border=0, patch=0)
    _, _, _, trace = run_ref(N, niter=12, **kw)
    assert len(trace) == 12 and min_gap(trace) > 1e-8 and len({s for s, _, _ in trace}) >= 2, trace
    psf, img, _ = fixture(N)
    for j in range(1, 13):
        gm, gr, gs = run_dev(ctx, N, niter=j, **kw)
        counts = [sum(1 for s, _, _ in trace[:j] if s == t) for t in range(6)]
        assert gs[0] == j and gs[3] == trace[j - 1][0] and gs[6:].tolist() == counts, (j, gs, trace[:j])
        wm, wr, ws, _ = run_ref(N, niter=j, **kw)
        compare((gm, gr, gs), (wm, wr, ws), np.abs(img).max(), f"N {N} prefix {j}")


def test_the_radius_31_halo(ctx):
    """scales [0, 32]: the widest kernel (63 x 63 taps) at N = 130 - three tile columns of the convolution, two of the
    iteration, and a kernel support that reaches over the image's edge"""
    N, scales = 130, [0.0, 32.0]
    psf, img, _ = fixture(N, scales)
    kw = dict(gain=0.25, threshold=0.0, niter=40, border=0, patch=0)
    want = run_ref(N, scales, **kw)
    assert min_gap(want[3]) > 1e-8 and 1 in {s for s, _, _ in want[3]}, want[2]
    compare(run_dev(ctx, N, scales, **kw), want, np.abs(img).max(), "scales [0, 32]")


@pytest.mark.parametrize("N", [96, 97, 200])
def test_the_delta_scale_alone_is_hogbom_bit_for_bit(ctx, N):
    psf, img, _ = fixture(N)
    assert psf[N // 2, N // 2] == 1.0
    for border, patch in ((0, 0), (N // 8, 20)):
        kw = dict(gain=0.2, threshold=0.0, niter=NITER, border=border, patch=patch)
        hm, hr, hs = (host(t) for t in ctx.clean(to_dev(img), to_dev(psf), **kw))
        gm, gr, gs = run_dev(ctx, N, [0.0], [1.0], **kw)
        assert np.array_equal(gm, hm) and np.array_equal(gr, hr)
        assert gs[0] == hs[0] == NITER and gs[1] == hs[1] and gs[2] == hs[2]
        # (the flux is a statistic, not part of the equivalence: msclean adds the rounded f, as its header says)
        assert abs(gs[4] - hs[3]) / np.abs(img).max() < TOL
        assert gs[3] == 0 and gs[6:].tolist() == [NITER, 0, 0, 0, 0, 0]


def test_host_dev_and_imager_forms_give_the_same_bits(ctx):
    """Host form == _dev form == Imager.msclean on the same arrays, bit for bit, and twice over (the second imager call
    takes the cross-PSFs it kept)."""
    c = Case(ctx, "w_cache", 0.1, 1290, 4000, 31)  # N = 129: odd, two tile columns
    psf = host(c.im.psf).copy()
    img = host(c.cycle(c.dvis))
    kw = dict(gain=0.2, threshold=0.0, niter=80, border=3, patch=0)
    outs = []
    for rep in range(2):
        a = img.copy()
        m, r, s = ctx.msclean(a, psf, SCALES, **kw)
        assert r is a
        outs.append((m, r, s))
        outs.append(tuple(host(t) for t in ctx.msclean(to_dev(img), to_dev(psf), SCALES, **kw)))
        outs.append(tuple(host(t) for t in c.im.msclean(to_dev(img), SCALES, **kw)))
    assert outs[0][2][0] == 80 and np.count_nonzero(outs[0][2][6:]) >= 2, outs[0][2]
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert np.array_equal(x, y)
    c.im.close()


def test_it_does_its_job(ctx):
    """At equal niter and gain the multi-scale residual rms is below half the Hogbom one on the extended fixture."""
    N = 96
    psf, img, _ = fixture(N)
    kw = dict(gain=0.2, threshold=0.0, niter=NITER, border=0, patch=0)
    wm, wr, ws, _ = run_ref(N, **kw)
    hr = img.copy()
    clean_ref.clean(psf, hr, np.zeros_like(hr), 0.2, 0.0, NITER)
    print(f"reference: multi-scale rms {wr.std():.4f}, hogbom rms {hr.std():.4f}, ratio {wr.std() / hr.std():.3f}")
    assert wr.std() < 0.5 * hr.std(), "precondition, on the reference"
    gm, gr, gs = run_dev(ctx, N, **kw)
    _, dr, _ = (host(t) for t in ctx.clean(to_dev(img), to_dev(psf), **kw))
    print(f"device: multi-scale rms {gr.std():.4f}, hogbom rms {dr.std():.4f}, per scale {gs[6:9]}")
    assert gr.std() < 0.5 * dr.std()
    assert np.count_nonzero(gs[6:]) >= 2


def test_stopped_early_the_trailing_launches_are_no_ops(ctx):
    """The threshold is reached after some of the 150 enqueued iterations: residual and model are exactly those of a
    call that enqueues just the iterations taken."""
    N = 97
    psf, img, _ = fixture(N)
    peak = np.abs(img).max()
    kw = dict(gain=0.25, threshold=0.3 * peak, niter=NITER, border=0, patch=0)
    want = run_ref(N, **kw)
    done = int(want[2][0])
    assert 0 < done < NITER, want[2]
    got = run_dev(ctx, N, **kw)
    compare(got, want, peak, "stopped early")
    exact = run_dev(ctx, N, **dict(kw, threshold=0.0, niter=done))
    assert np.array_equal(got[0], exact[0]) and np.array_equal(got[1], exact[1])
    assert np.array_equal(got[2], exact[2])


def test_model_is_accumulated_and_nan_is_never_selected(ctx):
    import torch
    N = 97
    psf, img, _ = fixture(N)
    bad = img.copy()
    bad[7, 9], bad[60, 40] = np.nan, np.nan
    kw = dict(gain=0.1, threshold=0.0, niter=60, border=0, patch=30)
    start = np.random.default_rng(5).normal(size=(N, N))
    wm, wr, ws, trace = run_ref(N, img=bad, start=start, **kw)
    assert min_gap(trace) > 1e-8 and ws[0] == 60
    dm = to_dev(start)
    m, r, s = ctx.msclean(to_dev(bad), to_dev(psf), SCALES, model=dm, **kw)
    assert m is dm
    gm, gr, gs = host(m), host(r), host(s)
    peak = np.nanmax(np.abs(bad))
    assert np.array_equal(gs[[0, 2, 3]], ws[[0, 2, 3]]) and np.array_equal(gs[5:], ws[5:])
    assert np.array_equal(np.isnan(gr), np.isnan(wr)) and np.isnan(gr).sum() == 2
    errs = (np.abs(gm - wm).max() / peak, np.nanmax(np.abs(gr - wr)) / peak, np.abs(gs - ws)[[1, 4]].max() / peak)
    print(f"accumulated, with NaN cells: model {errs[0]:.2e} residual {errs[1]:.2e} stats {errs[2]:.2e}")
    assert max(errs) < TOL
    # every searched cell NaN: nothing to select at any scale, nothing changes
    allnan = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda:0")
    m, r, s = ctx.msclean(allnan, to_dev(psf), SCALES, niter=5)
    gs = host(s)
    assert gs[0] == 0 and np.isnan(gs[1]) and gs[2] == -1 and gs[3] == -1 and not gs[4:].any() and not host(m).any()


def test_a_scale_whose_q_is_not_positive_is_never_chosen(ctx):
    """A PSF with a deep negative bowl around its peak: m_s (*) m_s (*) psf is negative at the centre for both wide
    scales, so only the delta can be taken - and with q_0 = b_0 = 1 the result is Hogbom's, bit for bit."""
    N = 96
    c = N // 2
    _, img, _ = fixture(N)
    yy, xx = np.mgrid[0:N, 0:N]
    psf = np.where((yy - c) ** 2 + (xx - c) ** 2 <= 64, -0.1, 0.0)
    psf[c, c] = 1.0
    _, _, q = msclean_ref.setup(psf, SCALES)
    assert q[0] == 1.0 and q[1] < 0 and q[2] < 0, q
    kw = dict(gain=0.1, threshold=0.0, niter=50, border=0, patch=0)
    gm, gr, gs = (host(t) for t in ctx.msclean(to_dev(img), to_dev(psf), SCALES, [1.0, 5.0, 5.0], **kw))
    hm, hr, hs = (host(t) for t in ctx.clean(to_dev(img), to_dev(psf), **kw))
    assert gs[0] == 50 and gs[6:].tolist() == [50, 0, 0, 0, 0, 0]
    assert np.array_equal(gm, hm) and np.array_equal(gr, hr)


@pytest.mark.parametrize("kind", ["simple", "w_cache"])
def test_deconvolve_is_the_loop_it_replaces(ctx, kind):
    import torch
    im, vis, N = point_sky(ctx, kind, 0.1, 640, 6000, 71)
    kw = dict(gain=0.2, threshold=0.0, niter=30, border=2, patch=0)
    dirty_peak = np.abs(host(im.cycle(vis))).max()

    def written_out(scales):
        m2 = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
        rows = []
        for cyc in range(3):
            img = im.cycle(vis, m2)
            _, _, s = im.msclean(img, scales, model=m2, **kw)
            rows.append(host(s))
        return host(m2), host(im.cycle(vis, m2)), np.array(rows)

    def check(scales, what):
        model, image, stats = im.deconvolve(vis, 3, scales=scales, **kw)
        gm, gi, gs = host(model), host(image), host(stats)
        wm, wi, ws = written_out(scales)
        mp, ip = np.abs(wm).max(), np.abs(wi).max()
        em, ei = np.abs(gm - wm).max() / mp, np.abs(gi - wi).max() / ip
        print(f"{kind} {what}: model {em:.2e} image {ei:.2e}")
        assert mp > 0 and em < TOL and ei < TOL
        assert gs.shape == (3, 12) and np.array_equal(gs[:, [0, 3]], ws[:, [0, 3]]) and np.array_equal(gs[:, 5:], ws[:, 5:])
        assert np.abs(gs - ws).max() / dirty_peak < TOL

    check([0.0, 2.5, 6.0], "first scales")
    # the same scales again: the imager kept the cross-PSFs and takes no memory
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    im.deconvolve(vis, 3, scales=[0.0, 2.5, 6.0], **kw)
    im.msclean(im.cycle(vis), [0.0, 2.5, 6.0], **kw)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free
    # other scales: the cross-PSFs are rebuilt, a longer list grows the scratch, and going back rebuilds again
    check([0.0, 3.0, 5.0], "other scales")
    check([0.0, 2.0, 4.0, 8.0], "a longer list")
    check([0.0, 2.5, 6.0], "the first again")
    # without scales it is the Hogbom deconvolve, as before
    _, _, st = im.deconvolve(vis, 2, **kw)
    assert tuple(st.shape) == (2, 4)
    im.close()


def test_msclean_and_deconvolve_can_be_captured_into_a_hip_graph(ctx):
    import torch
    im, vis, N = point_sky(ctx, "w_cache", 0.1, 640, 6000, 81)
    kw = dict(gain=0.2, threshold=0.0, niter=20, border=0, patch=16)
    scales = [0.0, 2.5, 6.0]
    img, model, dimg, dmodel = (torch.zeros((N, N), dtype=torch.float64, device="cuda:0") for _ in range(4))
    dirty = im.cycle(vis).clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream
        im.msclean(img, scales, model=model, **kw)
        im.deconvolve(vis, 2, model=dmodel, out=dimg, scales=scales, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, _, st = im.msclean(img, scales, model=model, **kw)
        _, _, dst = im.deconvolve(vis, 2, model=dmodel, out=dimg, scales=scales, **kw)
    torch.cuda.synchronize()
    for rep in range(2):
        img.copy_(dirty * (rep + 1))
        model.zero_()
        dmodel.zero_()
        dimg.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (model, img, st, dmodel, dimg, dst)]
        em, er, es = im.msclean(dirty * (rep + 1), scales, **kw)
        dm, di, ds = im.deconvolve(vis, 2, scales=scales, **kw)
        torch.cuda.synchronize()
        assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[3]) > 0
        for a, b in zip(got[:3], (em, er, es)):
            assert np.array_equal(a, host(b))
        peak = np.abs(host(dirty)).max()
        for a, b in zip(got[3:5], (dm, di)):
            assert np.abs(a - host(b)).max() / peak < TOL
        assert np.array_equal(got[5][:, [0, 3]], host(ds)[:, [0, 3]])
    assert ctx.get_option("errors") == 0
    im.close()


def test_another_call_between_two_mscleans_changes_nothing(ctx):
    N = 97
    kw = dict(gain=0.1, threshold=0.0, niter=40, border=0, patch=0)
    first = run_dev(ctx, N, **kw)
    u, v, w, vis = stream(2000, 490, 300.0, 44)
    ctx.do_imaging(0.1, 490, (to_dev(u), to_dev(v), to_dev(w)), None, None, None, None, to_dev(vis),
                   ("w_cache", {"wstep": 60, "qpx": 2, "npixFF": 16, "npixKern": 9}))
    psf, img, _ = fixture(N)
    ctx.clean(to_dev(img), to_dev(psf), niter=5)
    again = run_dev(ctx, N, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_refusals(ctx):
    """every argument rule the header adds to clean's, with its code, before anything is touched"""
    import torch
    import gridhip
    EINVAL, EUNSUPPORTED = gridhip._lib.EINVAL, gridhip._lib.EUNSUPPORTED
    N = 16
    psf, img, model = (torch.full((N, N), v, dtype=torch.float64, device="cuda:0") for v in (1.0, 2.0, 3.0))
    good = dict(gain=0.1, threshold=0.0, niter=5, border=0, patch=0)
    nan, inf = float("nan"), float("inf")
    bad = [([], None), ([0, 1, 2, 3, 4, 5, 6], None), ([1.0, 2.0], [1, 1]), ([0, 2, 2], [1, 1, 1]), ([0, 3, 2], [1, 1, 1]),
           ([0, nan], [1, 1]), ([nan], [1]), ([0, 2], [1, 0]), ([0, 2], [1, -1]), ([0, 2], [inf, 1]), ([0, 2], [1, nan])]
    lib, h = ctx._lib, ctx._h
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    arr = lambda v: (C.c_double * max(1, len(v)))(*v)  # noqa: E731
    def bound(entry):
        return lambda S, sc, bi, gain=0.1: entry(h, N, p(psf), p(img), p(model), S, sc, bi, gain, 0.0, 5, 0, 0, None)
    for form in (bound(lib.gridhip_msclean_dev), bound(lib.gridhip_msclean)):
        for sc, bi in bad:
            bi = [1.0] * len(sc) if bi is None else bi
            assert form(len(sc), arr(sc), arr(bi)) == EINVAL, (sc, bi)
        assert form(2, None, arr([1, 1])) == EINVAL and form(2, arr([0, 2]), None) == EINVAL
        assert form(2, arr([0, 32.5]), arr([1, 1])) == EUNSUPPORTED
        assert form(2, arr([0, 2]), arr([1, 1]), gain=0.0) == EINVAL  # clean's own rules still hold
    for kw_bad in (dict(gain=1.5), dict(niter=-1), dict(border=N // 2), dict(patch=-1), dict(threshold=-1.0)):
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.msclean(img, psf, [0, 2], model=model, **dict(good, **kw_bad))
        assert ei.value.code == EINVAL, kw_bad
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.msclean(img, psf, [0, 40], model=model, **good)
    assert ei.value.code == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((psf == 1.0).all()) and bool((img == 2.0).all()) and bool((model == 3.0).all())
    # niter = 0 is valid: nothing changes, the peak is reported; 32 cells is the largest scale taken
    m, r, s = ctx.msclean(img, psf, [0, 32], model=model, niter=0)
    assert host(s).tolist() == [0.0, 2.0, 0.0, -1.0] + [0.0] * 8
    assert bool((img == 2.0).all()) and bool((model == 3.0).all())
