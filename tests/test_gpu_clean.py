"""Deconvolution on the device (gridhip_clean*, gridhip_imager_clean_dev, gridhip_imager_deconvolve_dev) against the
numpy restatement of include/gridhip.h's definition (tests/clean_ref.py).

Tolerance: identical component positions and iteration counts; model, residual and stats within 1e-10 of the image's
peak, the bound the project uses everywhere (nothing here is accumulated with atomics, so agreement is expected to be
far tighter; each figure is printed before it is asserted).  Precondition, asserted on the reference alone: over all
iterations the relative gap between the two largest |residual| cells exceeds 1e-8 - with a smaller gap a last-bit
difference could legitimately change the component sequence."""
import ctypes as C

import numpy as np
import pytest

import clean_ref
from oracle import gridref_np as P
from test_gpu_imager import KO, Case, host, imgfn_of, stream, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-10


def inputs(N, seed=0):
    psf = clean_ref.make_psf(N, 100 + seed)
    img, _ = clean_ref.make_sky(psf, 200 + seed)
    return psf, img


def run_ref(psf, img, **kw):
    res, model, trace = img.copy(), np.zeros_like(img), []
    stats = clean_ref.clean(psf, res, model, kw["gain"], kw["threshold"], kw["niter"], kw["border"], kw["patch"], trace)
    return model, res, stats, trace


def run_dev(ctx, psf, img, **kw):
    m, r, s = ctx.clean(to_dev(img), to_dev(psf), **kw)
    return host(m), host(r), host(s)


def compare(got, want, peak, what):
    gm, gr, gs = got
    wm, wr, ws = want[:3]
    assert gs[0] == ws[0], f"{what}: {gs[0]} iterations, the reference {ws[0]}"
    assert gs[2] == ws[2], f"{what}: final peak at {gs[2]}, the reference {ws[2]}"
    assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(wm)), f"{what}: component positions differ"
    errs = (np.abs(gm - wm).max() / peak, np.abs(gr - wr).max() / peak, np.abs(gs - ws)[[1, 3]].max() / peak)
    print(f"{what}: model {errs[0]:.2e} residual {errs[1]:.2e} stats {errs[2]:.2e}")
    assert max(errs) < TOL, (what, errs)
    return errs


@pytest.mark.parametrize("gain", [0.1, 0.25])
@pytest.mark.parametrize("N", [256, 255, 600])
def test_against_the_restatement(ctx, N, gain):
    psf, img = inputs(N)
    peak = np.abs(img).max()
    worst, bits = 0.0, True
    for border in (0, N // 8):
        for patch in (0, 32):
            for threshold, midway in ((0.0, False), (0.5 * peak, True)):
                for niter in (0, 1, 400):
                    kw = dict(gain=gain, threshold=threshold, niter=niter, border=border, patch=patch)
                    want = run_ref(psf, img, **kw)
                    gaps = [g for _, g in want[3]]
                    assert not gaps or min(gaps) > 1e-8, f"precondition: smallest gap {min(gaps):.2e} (change the seed)"
                    if niter == 400:
                        # the two thresholds: one stops the loop midway, the other is never reached
                        assert (0 < want[2][0] < niter) if midway else want[2][0] == niter, want[2]
                    got = run_dev(ctx, psf, img, **kw)
                    errs = compare(got, want, peak, f"N {N} gain {gain} {kw}")
                    worst = max(worst, *errs)
                    bits = bits and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want[:3]))
    print(f"N {N} gain {gain}: worst {worst:.2e}, bit for bit {bits}")


def test_stopped_early_the_trailing_launches_are_no_ops(ctx):
    """The threshold is reached after a few components of 400 enqueued iterations: residual and model are exactly what
    the restatement leaves, which stops there."""
    N = 256
    psf, img = inputs(N, 1)
    peak = np.abs(img).max()
    kw = dict(gain=0.25, threshold=0.8 * peak, niter=400, border=0, patch=0)
    want = run_ref(psf, img, **kw)
    assert 0 < want[2][0] < 40, want[2]
    got = run_dev(ctx, psf, img, **kw)
    compare(got, want, peak, "stopped early")
    for a, b in zip(got, want[:3]):
        assert np.array_equal(a, b)


def test_model_is_accumulated_and_nan_is_never_selected(ctx):
    import torch
    N = 255
    psf, img = inputs(N, 2)
    img[7, 9], img[200, 100] = np.nan, np.nan
    kw = dict(gain=0.1, threshold=0.0, niter=60, border=0, patch=40)
    start = np.random.default_rng(5).normal(size=(N, N))
    res, model = img.copy(), start.copy()
    ws = clean_ref.clean(psf, res, model, kw["gain"], kw["threshold"], kw["niter"], kw["border"], kw["patch"])
    dm = to_dev(start)
    m, r, s = ctx.clean(to_dev(img), to_dev(psf), model=dm, **kw)
    assert m is dm
    gm, gr, gs = host(m), host(r), host(s)
    peak = np.nanmax(np.abs(img))
    assert gs[0] == ws[0] == 60 and gs[2] == ws[2]
    assert np.nanmax(np.abs(gr - res)) / peak < TOL and np.array_equal(np.isnan(gr), np.isnan(res))
    assert np.abs(gm - model).max() / peak < TOL and np.abs(gs - ws).max() / peak < TOL
    # every searched cell NaN: nothing to select, nothing changes
    allnan = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda:0")
    m, r, s = ctx.clean(allnan, to_dev(psf), niter=5)
    gs = host(s)
    assert gs[0] == 0 and np.isnan(gs[1]) and gs[2] == -1 and gs[3] == 0 and not host(m).any()


def test_host_dev_and_imager_forms_give_the_same_bits(ctx):
    """Host form == _dev form == Imager.clean on the same arrays, bit for bit, and twice over: the path is deterministic
    by construction."""
    theta, lam = 0.1, 1290  # N = 129: odd, two tile columns
    c = Case(ctx, "w_cache", theta, lam, 4000, 31)
    N = c.N
    psf = host(c.im.psf).copy()
    img = host(c.cycle(c.dvis))
    kw = dict(gain=0.2, threshold=0.0, niter=120, border=3, patch=0)
    outs = []
    for rep in range(2):
        a = img.copy()
        m, r, s = ctx.clean(a, psf, **kw)
        assert r is a
        outs.append((m, r, s))
        outs.append(tuple(host(t) for t in ctx.clean(to_dev(img), to_dev(psf), **kw)))
        outs.append(tuple(host(t) for t in c.im.clean(to_dev(img), **kw)))
    assert outs[0][2][0] == 120 and np.count_nonzero(outs[0][0]) > 1
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert np.array_equal(x, y)
    want = run_ref(psf, img, **kw)
    assert min(g for _, g in want[3]) > 1e-8
    compare(outs[0], want, np.abs(img).max(), "imager psf")
    c.im.close()


def bump(S):
    g = np.exp(-0.5 * ((np.arange(S) - S // 2) / 1.5) ** 2)
    return np.outer(g, g).astype(np.complex128)


@pytest.mark.parametrize("theta,lam", [(0.1, 640), (0.1, 490)])  # N = 64 and N = 49
@pytest.mark.parametrize("kind", ["simple", "conv", "w_cache", "aw"])
def test_an_imagers_psf_peaks_at_the_centre(ctx, kind, theta, lam):
    """The zero-lag cell of an imager's PSF is (N / 2, N / 2) for every imaging kind, even and odd N: the cell clean
    takes as the PSF's centre.  The conv and aw kernels are positive bumps, as gridding kernels are (a table of random
    numbers tapers the image by a random pattern, which may lift a sidelobe above the centre)."""
    N, n, A = P.haskell_round(theta * lam), 3000, 4
    u, v, w, _ = stream(n, lam, 100.0, 17)
    duvw = tuple(to_dev(x) for x in (u, v, w))
    rng = np.random.default_rng(18)
    a1 = a2 = None
    if kind == "conv":
        imgfn = ("conv", to_dev(np.broadcast_to(bump(7), (4, 4, 7, 7))))
    elif kind == "aw":
        imgfn = ("aw", to_dev(np.broadcast_to(bump(9), (3, 2, 2, 9, 9))), to_dev(np.linspace(-100.0, 100.0, 3)),
                 to_dev(np.broadcast_to(bump(9), (A, 9, 9))))
        a1, a2 = to_dev(rng.integers(0, A, n)), to_dev(rng.integers(0, A, n))
    else:
        imgfn = imgfn_of(kind)
    im = ctx.imager(theta, lam, duvw, imgfn, a1=a1, a2=a2)
    psf = host(im.psf)
    assert int(np.argmax(psf)) == (N // 2) * N + N // 2 and psf[N // 2, N // 2] == 1.0
    im.close()


def point_sky(ctx, kind, theta, lam, n, seed):
    """an imager and the visibilities of a few point sources predicted through it"""
    import torch
    N = P.haskell_round(theta * lam)
    u, v, w, _ = stream(n, lam, 100.0, seed, span=0.3)
    duvw = tuple(to_dev(x) for x in (u, v, w))
    im = ctx.imager(theta, lam, duvw, ("w_cache", KO) if kind == "w_cache" else ("simple",))
    sky = np.zeros((N, N))
    rng = np.random.default_rng(seed + 1)
    for _ in range(4):
        sky[rng.integers(N // 4, N - N // 4), rng.integers(N // 4, N - N // 4)] = rng.uniform(0.5, 1.0)
    vis = im.predict(to_dev(sky))
    torch.cuda.synchronize()
    return im, vis, N


@pytest.mark.parametrize("kind", ["simple", "w_cache"])
def test_deconvolve_is_the_loop_it_replaces(ctx, kind):
    import torch
    im, vis, N = point_sky(ctx, kind, 0.1, 640, 6000, 71)
    kw = dict(gain=0.2, threshold=0.0, niter=40, border=2, patch=0)
    model, image, stats = im.deconvolve(vis, 3, **kw)
    # the same, written out
    m2 = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    rows, first = [], None
    for cyc in range(3):
        img = im.cycle(vis, m2)
        if first is None:
            first = host(img).copy()
        _, _, s = im.clean(img, m2, **kw)
        rows.append(host(s))
    closing = host(im.cycle(vis, m2))
    gm, gi, gs = host(model), host(image), host(stats)
    mp, ip = np.abs(host(m2)).max(), np.abs(closing).max()
    em, ei = np.abs(gm - host(m2)).max() / mp, np.abs(gi - closing).max() / ip
    print(f"{kind}: model {em:.2e} image {ei:.2e}; dirty peak {np.abs(first).max():.4g}, closing {ip:.4g}")
    assert mp > 0 and em < TOL and ei < TOL
    assert gs.shape == (3, 4) and np.array_equal(gs[:, 0], [r[0] for r in rows])
    assert np.abs(gs - np.array(rows)).max() / np.abs(first).max() < TOL
    assert ip < np.abs(first).max()  # the closing residual image's peak fell below the first dirty image's
    im.close()


def test_clean_and_deconvolve_can_be_captured_into_a_hip_graph(ctx):
    import torch
    im, vis, N = point_sky(ctx, "w_cache", 0.1, 640, 6000, 81)
    kw = dict(gain=0.2, threshold=0.0, niter=30, border=0, patch=16)
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    model = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    dimg = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    dmodel = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    dirty = im.cycle(vis).clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream
        im.clean(img, model, **kw)
        im.deconvolve(vis, 2, model=dmodel, out=dimg, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        _, _, st = im.clean(img, model, **kw)
        _, _, dst = im.deconvolve(vis, 2, model=dmodel, out=dimg, **kw)
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
        em, er, es = im.clean(dirty * (rep + 1), None, **kw)
        dm, di, ds = im.deconvolve(vis, 2, **kw)
        torch.cuda.synchronize()
        assert np.count_nonzero(got[0]) > 0 and np.count_nonzero(got[3]) > 0
        for a, b in zip(got[:3], (em, er, es)):
            assert np.array_equal(a, host(b))
        peak = np.abs(host(dirty)).max()
        for a, b in zip(got[3:], (dm, di, ds)):
            assert np.abs(a - host(b)).max() / peak < TOL
    assert ctx.get_option("errors") == 0
    im.close()


def test_another_call_between_two_cleans_changes_nothing(ctx):
    N = 256
    psf, img = inputs(N, 3)
    kw = dict(gain=0.1, threshold=0.0, niter=50, border=0, patch=0)
    first = run_dev(ctx, psf, img, **kw)
    u, v, w, vis = stream(2000, 490, 300.0, 44)
    ctx.do_imaging(0.1, 490, (to_dev(u), to_dev(v), to_dev(w)), None, None, None, None, to_dev(vis),
                   ("w_cache", {"wstep": 60, "qpx": 2, "npixFF": 16, "npixKern": 9}))
    again = run_dev(ctx, psf, img, **kw)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_refusals(ctx):
    """every argument rule of the header, GRIDHIP_EINVAL, before anything is touched"""
    import torch
    import gridhip
    N = 16
    psf, img, model = (torch.full((N, N), v, dtype=torch.float64, device="cuda:0") for v in (1.0, 2.0, 3.0))
    good = dict(gain=0.1, threshold=0.0, niter=5, border=0, patch=0)
    bad = [dict(gain=0.0), dict(gain=1.5), dict(gain=float("nan")), dict(threshold=-1.0), dict(threshold=float("nan")),
           dict(niter=-1), dict(border=-1), dict(border=N // 2), dict(patch=-1)]
    for b in bad:
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.clean(img, psf, model=model, **dict(good, **b))
        assert ei.value.code == gridhip._lib.EINVAL, b
    big = torch.full((2 * N * N,), 4.0, dtype=torch.float64, device="cuda:0")
    lib, h = ctx._lib, ctx._h
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    calls = [(0, p(psf), p(img), p(model)), (N, None, p(img), p(model)), (N, p(psf), None, p(model)),
             (N, p(psf), p(img), None), (N, p(psf), p(img), p(img)), (N, p(psf), p(psf), p(model)),
             (N, p(big), p(big, 8 * (N * N - 1)), p(model))]  # the last: residual overlaps psf by one cell
    for form in (lib.gridhip_clean_dev, lib.gridhip_clean):
        for n_, a, b, c_ in calls:
            assert form(h, n_, a, b, c_, 0.1, 0.0, 5, 0, 0, None) == gridhip._lib.EINVAL
    torch.cuda.synchronize()
    assert bool((psf == 1.0).all()) and bool((img == 2.0).all()) and bool((model == 3.0).all()) and bool((big == 4.0).all())
    # niter = 0 is valid: nothing changes, the peak is reported
    m, r, s = ctx.clean(img, psf, model=model, niter=0)
    assert host(s).tolist() == [0.0, 2.0, 0.0, 0.0] and bool((img == 2.0).all()) and bool((model == 3.0).all())
