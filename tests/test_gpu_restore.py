"""The restoring beam and the restore on the device (gridhip_fit_beam*, gridhip_restore*, gridhip_imager_beam_dev,
gridhip_imager_restore_dev) against the numpy restatement of include/gridhip.h's definition (tests/restore_ref.py).

Tolerances, derived and not measured.
Fit: ncells and ok equal; A, B, C within 1e-9 relative (of the largest of the three).  The device's log and numpy's
differ by a few ulp over at most 4 224 terms and the solve amplifies that by the condition number of the 3 x 3 system,
which is computed and printed for every input; the bound widens to 1e-16 x 4 224 x condition number only where that
exceeds 1e-9.  For the generated PSFs the restatement alone gives condition numbers of 1.5 to 19, so 1e-9 applies;
an imager's PSF has its own, printed with the rest, and the same rule.
bmaj, bmin and bpa are compared with the header's formulas applied to the device's own A, B, C, at 1e-12.
Restore: per cell |gpu - ref| <= 1e-12 x (|residual| + sum |model| beam): at most 4 225 products plus one addition in
fp64 and exp within a few ulp give (4 226 + 4) x 2^-53 = 4.7e-13."""
import ctypes as C

import numpy as np
import pytest

import clean_ref
import restore_ref
from test_gpu_clean import point_sky
from test_gpu_imager import KINDS, Case, host, stream, to_dev

pytestmark = pytest.mark.gpu
FIT_TOL, RESTORE_TOL = 1e-9, 1e-12


def fit_psfs():
    yield "smooth round 255", restore_ref.smooth_psf(255, 1, 0.15)
    yield "smooth round 256", restore_ref.smooth_psf(256, 1, 0.15)
    yield "smooth ellipse 255", restore_ref.smooth_psf(255, 2, 0.1, 0.5, 0.3)
    yield "smooth ellipse 256", restore_ref.smooth_psf(256, 2, 0.1, 0.5, 0.3)
    for N in (256, 255, 600):
        for seed in (1, 2, 3):
            yield f"sharp {N} seed {seed}", clean_ref.make_psf(N, seed)


def check_fit(what, got, psf, window, cut):
    want = restore_ref.fit_beam(psf, window, cut)
    M, _, _, _ = restore_ref.normal_equations(psf, window, cut)
    cond = np.linalg.cond(M) if want[7] else float("nan")
    tol = max(FIT_TOL, 1e-16 * 4224 * cond) if want[7] else FIT_TOL
    print(f"{what}: ncells {got[6]:.0f} ok {got[7]:.0f} condition number {cond:.3g} -> bound {tol:.2e}"
          f" ({'1e-9' if tol == FIT_TOL else 'widened'})")
    assert got[6] == want[6] and got[7] == want[7], (what, got, want)
    if not want[7]:
        assert np.all(np.isnan(got[:6]))
        return
    err = np.abs(got[:3] - want[:3]).max() / np.abs(want[:3]).max()
    print(f"{what}: A, B, C off by {err:.2e}; FWHM {got[3]:.3f} x {got[4]:.3f} cells at {got[5]:.3f} rad")
    assert err <= tol, (what, err)
    bmaj, bmin, bpa = restore_ref.derived(*got[:3])
    assert abs(got[3] - bmaj) <= 1e-12 * bmaj and abs(got[4] - bmin) <= 1e-12 * bmin and abs(got[5] - bpa) <= 1e-12
    assert got[3] >= got[4] and -np.pi / 2 < got[5] <= np.pi / 2


def test_fit_against_the_restatement(ctx):
    for what, psf in fit_psfs():
        for window, cut in ((8, 0.5), (32, 0.2)):
            dev = host(ctx.fit_beam(to_dev(psf), window, cut))
            check_fit(f"{what} window {window} cut {cut}", dev, psf, window, cut)
            hst = ctx.fit_beam(psf, window, cut)
            assert np.array_equal(dev, hst, equal_nan=True), "host and _dev forms differ"
    # a window beyond one pass of the kernel (128 rows) and beyond the grid's edge; a fit that fails
    psf = restore_ref.smooth_psf(600, 3, 0.02, 0.7, 1.0)
    for window in (100, 1000):
        check_fit(f"wide window {window}", host(ctx.fit_beam(to_dev(psf), window, 0.3)), psf, window, 0.3)
    bad = np.full((64, 64), -0.1)
    bad[32, 32] = 1.0
    check_fit("no usable neighbour", host(ctx.fit_beam(to_dev(bad))), bad, 8, 0.5)
    bad[32, 33] = bad[32, 31] = 0.6
    check_fit("two cells", host(ctx.fit_beam(to_dev(bad))), bad, 8, 0.5)
    tiny = np.ones((1, 1))
    check_fit("N = 1", host(ctx.fit_beam(to_dev(tiny))), tiny, 8, 0.5)


@pytest.mark.parametrize("theta,lam", [(0.1, 640), (0.1, 490)])  # N = 64 and N = 49
@pytest.mark.parametrize("kind", KINDS)
def test_fit_of_an_imagers_own_psf(ctx, kind, theta, lam):
    c = Case(ctx, kind, theta, lam, 3000, 23, bad_antennas=False)
    psf = host(c.im.psf).copy()
    got = host(c.im.beam())
    check_fit(f"imager {kind} N {c.N}", got, psf, 8, 0.5)
    assert np.array_equal(got, host(ctx.fit_beam(c.im.psf)), equal_nan=True)
    assert np.array_equal(got, host(c.im.beam(8, 0.5)), equal_nan=True)
    c.im.close()


def models(N, seed):
    rng = np.random.default_rng(seed)
    empty = np.zeros((N, N))
    corner = np.zeros((N, N))
    corner[N - 1, 0] = 1.5
    comps = np.zeros((N, N))
    comps[rng.integers(0, N, 25), rng.integers(0, N, 25)] = rng.uniform(0.2, 1.0, 25) * rng.choice([-1.0, 1.0], 25)
    dense = rng.normal(size=(N, N))
    return {"empty": empty, "corner": corner, "25 components": comps, "dense": dense}


BEAMS = {1: [0.9, 0.2, 1.4], 8: [0.11, 0.02, 0.19], 32: [0.012, -0.004, 0.02]}  # A, B, C that fill each support


@pytest.mark.parametrize("support", [1, 8, 32])
@pytest.mark.parametrize("N", [256, 255, 600])
def test_restore_against_the_restatement(ctx, N, support):
    beam = np.array(BEAMS[support] + [0.0, 0.0, 0.0, 8.0, 1.0])
    rng = np.random.default_rng(N + support)
    res = rng.normal(size=(N, N)) * 1e-2
    res[5, 7] = -0.0
    dbeam, dres = to_dev(beam), to_dev(res)
    for what, model in models(N, 7 * N + support).items():
        want, mag = restore_ref.restore(model, res, beam, support)
        got = host(ctx.restore(to_dev(model), dres, dbeam, support))
        worst = (np.abs(got - want)[mag > 0] / mag[mag > 0]).max()
        print(f"N {N} support {support} {what}: worst |gpu - ref| / magnitude {worst:.2e}")
        assert np.all(np.abs(got - want) <= RESTORE_TOL * mag), (what, worst)
        if what == "empty":
            assert np.array_equal(got, res) and not np.signbit(got[5, 7])  # residual + 0.0: -0.0 comes back as +0.0


def test_the_forms_give_the_same_bits_and_so_do_two_runs(ctx):
    theta, lam = 0.1, 1290  # N = 129: odd, three tile columns
    c = Case(ctx, "w_cache", theta, lam, 4000, 31)
    N = c.N
    psf = host(c.im.psf).copy()
    rng = np.random.default_rng(3)
    model = np.zeros((N, N))
    model[rng.integers(0, N, 40), rng.integers(0, N, 40)] = rng.normal(size=40)
    res = rng.normal(size=(N, N))
    outs = []
    for rep in range(2):
        beam = ctx.fit_beam(psf)
        assert beam[7] == 1.0
        outs.append(ctx.restore(model, res, beam, 6))
        dbeam = ctx.fit_beam(to_dev(psf))
        assert np.array_equal(host(dbeam), beam)
        outs.append(host(ctx.restore(to_dev(model), to_dev(res), dbeam, 6)))
        o, b = c.im.restore(to_dev(model), to_dev(res), support=6)
        assert np.array_equal(host(b), beam)
        outs.append(host(o))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    want, mag = restore_ref.restore(model, res, ctx.fit_beam(psf), 6)
    assert np.all(np.abs(outs[0] - want) <= RESTORE_TOL * mag)
    # support=None reads the beam back: the same image as the support it derives
    from gridhip._marshal import beam_support
    R = beam_support(ctx.fit_beam(psf))
    o, _ = c.im.restore(to_dev(model), to_dev(res))
    assert np.array_equal(host(o), host(ctx.restore(to_dev(model), to_dev(res), to_dev(ctx.fit_beam(psf)), R)))
    # in place: restored is the residual itself
    dres = to_dev(res)
    o = ctx.restore(to_dev(model), dres, to_dev(ctx.fit_beam(psf)), 6, out=dres)
    assert o is dres and np.array_equal(host(dres), outs[0])
    hres = res.copy()
    assert ctx.restore(model, hres, ctx.fit_beam(psf), 6, out=hres) is hres and np.array_equal(hres, outs[0])
    c.im.close()


def test_skipped_tiles_give_the_bits_of_the_full_sum(ctx):
    """The work-group skips the taps when its window holds no non-zero cell.  A tile-sparse model - components in one
    corner only, so that most tiles are skipped - against the same model plus one far-away component, which changes
    nothing within `support` of the first ones: the cells near them must have the same bits, and the far tiles are
    residual + 0.0 in the one and the full sum in the other.  And a dense model with exact zeros (of both signs)
    scattered in against the restatement, where no tile is skipped."""
    N, s = 600, 8
    beam = to_dev(np.array(BEAMS[8] + [0, 0, 0, 8.0, 1.0]))
    rng = np.random.default_rng(11)
    res = rng.normal(size=(N, N))
    res[300, 300] = -0.0
    sparse = np.zeros((N, N))
    sparse[rng.integers(0, 40, 12), rng.integers(0, 40, 12)] = rng.normal(size=12)
    far = sparse.copy()
    far[500, 500] = 3.0
    a = host(ctx.restore(to_dev(sparse), to_dev(res), beam, s))
    b = host(ctx.restore(to_dev(far), to_dev(res), beam, s))
    near = np.ones((N, N), dtype=bool)
    near[500 - s:500 + s + 1, 500 - s:500 + s + 1] = False
    assert np.array_equal(a[near], b[near]) and not np.array_equal(a, b)
    assert np.array_equal(a[100:, 100:], res[100:, 100:]) and not np.signbit(a[300, 300])
    # a model of zeros of both signs only: every tile is skipped, and equals what the taps would give
    signed = np.zeros((N, N))
    signed[::3, ::5] = -0.0
    z = host(ctx.restore(to_dev(signed), to_dev(res), beam, s))
    assert np.array_equal(z, res + 0.0) and not np.signbit(z[300, 300])
    dense = rng.normal(size=(N, N))
    dense[rng.random((N, N)) < 0.3] = 0.0
    dense[rng.random((N, N)) < 0.05] = -0.0
    dense[200:300, 100:420] = 0.0  # a block of whole tiles without a non-zero cell, inside a dense model
    want, mag = restore_ref.restore(dense, res, host(beam), s)
    got = host(ctx.restore(to_dev(dense), to_dev(res), beam, s))
    assert np.all(np.abs(got - want) <= RESTORE_TOL * mag)
    assert np.array_equal(got[210:290, 110:410], res[210:290, 110:410] + 0.0)


def test_a_failed_or_nan_beam(ctx):
    import gridhip
    N = 100
    rng = np.random.default_rng(2)
    model, res = rng.normal(size=(N, N)), rng.normal(size=(N, N))
    nan = float("nan")
    for beam in ([nan] * 6 + [2.0, 0.0], [0.2, 0.0, 0.3, 0, 0, 0, 8.0, 0.0], [nan, 0.0, 0.3, 0, 0, 0, 8.0, 1.0],
                 [0.2, 0.5, 0.3, 0, 0, 0, 8.0, 1.0], [0.2, 0.0, float("inf"), 0, 0, 0, 8.0, 1.0],
                 [-0.2, 0.0, 0.3, 0, 0, 0, 8.0, 1.0], [0.2, 0.0, 0.3, 0, 0, 0, 8.0, nan]):
        beam = np.array(beam, dtype=np.float64)
        out = host(ctx.restore(to_dev(model), to_dev(res), to_dev(beam), 4))
        assert np.all(np.isnan(out)), beam
        keep = np.full((N, N), 5.0)
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.restore(model, res, beam, 4, out=keep)
        assert ei.value.code == gridhip._lib.EINVAL and np.all(keep == 5.0), beam
    # a PSF whose fit fails, through the imager-free chain on the device: nothing is read back, the image is NaN
    bad = np.full((N, N), -0.1)
    bad[N // 2, N // 2] = 1.0
    db = ctx.fit_beam(to_dev(bad))
    assert np.all(np.isnan(host(ctx.restore(to_dev(model), to_dev(res), db, 4))))
    with pytest.raises(ValueError):
        ctx.restore(to_dev(model), to_dev(res), db)  # support=None reads the beam back and finds the fit failed


def test_deconvolve_then_restore_is_one_chain_and_can_be_captured(ctx):
    import torch
    im, vis, N = point_sky(ctx, "w_cache", 0.1, 640, 6000, 91)
    kw = dict(gain=0.2, threshold=0.0, niter=30, border=2, patch=0)
    s = 5
    # the chain, then the separate calls with another call on the context in between
    model, image, _ = im.deconvolve(vis, 2, **kw)
    restored, beam = im.restore(model, image, support=s)
    m2, i2, _ = im.deconvolve(vis, 2, **kw)
    u, v, w, ovis = stream(2000, 490, 300.0, 44)
    ctx.do_imaging(0.1, 490, (to_dev(u), to_dev(v), to_dev(w)), None, None, None, None, to_dev(ovis),
                   ("w_cache", {"wstep": 60, "qpx": 2, "npixFF": 16, "npixKern": 9}))
    b2 = ctx.fit_beam(im.psf)
    ctx.clean(torch.ones((32, 32), dtype=torch.float64, device="cuda:0"), torch.ones((32, 32), dtype=torch.float64,
                                                                                      device="cuda:0"), niter=2)
    r2 = ctx.restore(m2, i2, b2, s)
    assert np.array_equal(host(beam), host(b2)) and host(beam)[7] == 1.0
    peak = np.abs(host(restored)).max()
    assert np.abs(host(restored) - host(r2)).max() <= 1e-10 * peak  # (deconvolve's cycles use fp64 atomics)
    want, mag = restore_ref.restore(host(model), host(image), host(beam), s)
    assert np.all(np.abs(host(restored) - want) <= RESTORE_TOL * mag)
    assert np.count_nonzero(host(model)) > 0
    # captured: deconvolve + an in-place restore in one graph, replayed
    gm = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    gi = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    gr = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream
        im.deconvolve(vis, 2, model=gm, out=gi, **kw)
        im.restore(gm, gi, support=s, out=gr)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        im.deconvolve(vis, 2, model=gm, out=gi, **kw)
        _, gb = im.restore(gm, gi, support=s, out=gr)
    torch.cuda.synchronize()
    for rep in range(2):
        gm.zero_()
        gi.zero_()
        gr.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(gb), host(beam))
        # the restore of the replayed model and residual, eagerly: the same bits
        assert np.array_equal(host(gr), host(ctx.restore(gm, gi, gb, s)))
        assert np.abs(host(gr) - host(restored)).max() <= 1e-10 * peak
    assert ctx.get_option("errors") == 0
    im.close()


def test_refusals(ctx):
    """every argument rule of the header, before anything is touched"""
    import torch
    import gridhip
    EINVAL, EUNSUPPORTED = gridhip._lib.EINVAL, gridhip._lib.EUNSUPPORTED
    N = 16
    psf, model, res, out = (torch.full((N, N), v, dtype=torch.float64, device="cuda:0") for v in (1.0, 2.0, 3.0, 4.0))
    beam = torch.tensor([0.2, 0.0, 0.3, 0, 0, 0, 8.0, 1.0], dtype=torch.float64, device="cuda:0")
    big = torch.full((2 * N * N,), 6.0, dtype=torch.float64, device="cuda:0")
    hbeam = np.array([0.2, 0.0, 0.3, 0, 0, 0, 8.0, 1.0])
    lib, h = ctx._lib, ctx._h
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    nan = float("nan")
    for form in (lib.gridhip_fit_beam_dev, lib.gridhip_fit_beam):
        for n_, a, window, cut, b in ((0, p(psf), 8, 0.5, p(beam)), (N, None, 8, 0.5, p(beam)), (N, p(psf), 8, 0.5, None),
                                      (N, p(psf), 0, 0.5, p(beam)), (N, p(psf), -3, 0.5, p(beam)),
                                      (N, p(psf), 8, 0.0, p(beam)), (N, p(psf), 8, 1.0, p(beam)),
                                      (N, p(psf), 8, -0.5, p(beam)), (N, p(psf), 8, nan, p(beam)),
                                      (N, p(big), 8, 0.5, p(big, 8 * (N * N - 1)))):
            assert form(h, n_, a, window, cut, b) == EINVAL, (n_, window, cut)
    hb = C.c_void_p(hbeam.ctypes.data)
    for form, b in ((lib.gridhip_restore_dev, p(beam)), (lib.gridhip_restore, hb)):
        for n_, m, r, bb, sup, o in ((0, p(model), p(res), b, 4, p(out)), (N, None, p(res), b, 4, p(out)),
                                     (N, p(model), None, b, 4, p(out)), (N, p(model), p(res), None, 4, p(out)),
                                     (N, p(model), p(res), b, 4, None), (N, p(model), p(res), b, 0, p(out)),
                                     (N, p(model), p(res), b, -1, p(out)), (N, p(model), p(res), b, 4, p(model)),
                                     (N, p(big), p(res), b, 4, p(big, 8 * (N * N - 1))),   # restored overlaps model
                                     (N, p(model), p(big), b, 4, p(big, 8))):              # ... residual, shifted
            assert form(h, n_, m, r, bb, sup, o) == EINVAL, (n_, sup)
        assert form(h, N, p(model), p(res), b, 33, p(out)) == EUNSUPPORTED
    # the Python methods raise with the library's code; an imager's forms check the same rules
    with pytest.raises(gridhip.GridHipError) as ei:
        ctx.restore(model, res, beam, 33, out=out)
    assert ei.value.code == EUNSUPPORTED
    for kw in (dict(window=0), dict(cut=0.0), dict(cut=1.0), dict(cut=nan)):
        with pytest.raises(gridhip.GridHipError) as ei:
            ctx.fit_beam(psf, **kw)
        assert ei.value.code == EINVAL, kw
    c = Case(ctx, "simple", 0.1, 160, 500, 5)
    n = c.N
    im_m, im_r, im_o = (torch.full((n, n), v, dtype=torch.float64, device="cuda:0") for v in (2.0, 3.0, 4.0))
    ih = c.im._h
    for args in ((None, p(im_r), 8, 0.5, 4, p(im_o), p(beam)), (p(im_m), None, 8, 0.5, 4, p(im_o), p(beam)),
                 (p(im_m), p(im_r), 8, 0.5, 4, None, p(beam)), (p(im_m), p(im_r), 0, 0.5, 4, p(im_o), p(beam)),
                 (p(im_m), p(im_r), 8, 1.5, 4, p(im_o), p(beam)), (p(im_m), p(im_r), 8, 0.5, 0, p(im_o), p(beam)),
                 (p(im_m), p(im_r), 8, 0.5, 4, p(im_m), p(beam))):
        assert lib.gridhip_imager_restore_dev(ih, *args) == EINVAL, args[2:5]
    assert lib.gridhip_imager_restore_dev(ih, p(im_m), p(im_r), 8, 0.5, 33, p(im_o), None) == EUNSUPPORTED
    assert lib.gridhip_imager_beam_dev(ih, 0, 0.5, p(beam)) == EINVAL
    assert lib.gridhip_imager_beam_dev(ih, 8, 0.5, None) == EINVAL
    torch.cuda.synchronize()
    for t, v in ((psf, 1.0), (model, 2.0), (res, 3.0), (out, 4.0), (big, 6.0), (im_m, 2.0), (im_r, 3.0), (im_o, 4.0)):
        assert bool((t == v).all()), v
    assert np.array_equal(host(beam), hbeam)
    # the beam output of the imager form may be NULL
    assert lib.gridhip_imager_restore_dev(ih, p(im_m), p(im_r), 8, 0.5, 4, p(im_o), None) == 0
    torch.cuda.synchronize()
    c.im.close()
