"""Wide-band imagers on the GPU (gridhip_imager_set_spectral_dev, _spectral_psfs_dev, _mfs_cycle_dev, _mfclean_dev,
_mfdeconvolve_dev): every call against the composition of existing calls that include/gridhip.h ("wide-band imaging")
defines it by, on the small cases of test_gpu_imager.py (theta 0.1, lam 1290, N = 129), every imaging kind, T = 2.

Tolerance: 1e-10 of the reference's largest magnitude, the project's bound wherever a scatter is involved (its fp64
atomics make no two passes over the same visibilities agree bit for bit - which is also why mfdeconvolve is compared with
the loop it is defined by to this bound, with identical iteration counts and component positions, and not bit for bit:
both sides grid their residuals through the atomics); 1e-12 for an imager against itself."""
import numpy as np
import pytest

from test_gpu_imager import KINDS, Case, host, rel, to_dev

pytestmark = pytest.mark.gpu
TOL = 1e-10
THETA, LAM, T = 0.1, 1290, 2
CHANNELS = np.linspace(-0.2, 0.2, 8)


def spectral_case(ctx, kind, n=3000, seed=11, bad=()):
    """a Case with T = 2 terms: x drawn from eight channel values; `bad`: (index, value) pairs of non-finite x"""
    c = Case(ctx, kind, THETA, LAM, n, seed, bad_antennas=False)
    x = np.random.default_rng(seed + 5).choice(CHANNELS, n)
    for k, v in bad:
        x[k] = v
    c.x, c.dx = x, to_dev(x)
    c.im.set_spectral(c.dx, T)
    return c


def composed(c, vis, models, x, flagged=None):
    """mfs_cycle written out with Imager.predict and Imager.cycle: (images, r); flagged: the visibilities that predict 0
    and grid nothing"""
    import torch
    r = vis.clone()
    keep = None if flagged is None else ~flagged
    if models is not None:
        for q in range(T):
            p = x ** q * c.im.predict(models[q])
            r = r - (p if keep is None else torch.where(keep, p, torch.zeros_like(p)))
    imgs = []
    for t in range(T):
        v = x ** t * r
        imgs.append(c.im.cycle((v if keep is None else torch.where(keep, v, torch.zeros_like(v))).contiguous()))
    return torch.stack(imgs), r


@pytest.mark.parametrize("kind", KINDS)
def test_spectral_psfs_and_mfs_cycle_against_the_calls_they_are_defined_by(ctx, kind):
    import torch
    c = spectral_case(ctx, kind)
    assert c.N == 129
    psfs = host(c.im.spectral_psfs())
    assert psfs.shape == (2 * T - 1, c.N, c.N)
    figs = {"P_0 vs psf": np.abs(psfs[0] - host(c.im.psf)).max()}
    for s in range(2 * T - 1):
        want = host(c.im.cycle((c.dx ** s).to(torch.complex128)))
        figs[f"P_{s}"] = np.abs(psfs[s] - want).max()  # (in units of pmax: the PSF's own peak is 1)
    models = to_dev(np.random.default_rng(3).normal(size=(T, c.N, c.N)))
    vis_res = torch.full_like(c.dvis, 7.0)
    got = c.im.mfs_cycle(c.dvis, models, vis_res=vis_res)
    want, r = composed(c, c.dvis, models, c.dx)
    figs["images"] = rel(host(got), host(want))
    figs["vis_res"] = rel(host(vis_res), host(r))
    buf = c.dvis.clone()
    figs["images, in place"] = rel(host(c.im.mfs_cycle(buf, models, vis_res=buf)), host(want))
    figs["vis_res, in place"] = rel(host(buf), host(r))
    # without models: T plain cycles, and vis_res receives vis
    same = torch.full_like(c.dvis, 7.0)
    got0 = c.im.mfs_cycle(c.dvis, vis_res=same)
    want0, _ = composed(c, c.dvis, None, c.dx)
    figs["images, no models"] = rel(host(got0), host(want0))
    print(kind, figs)
    assert np.abs(host(want)).max() > 0 and np.abs(psfs[1]).max() > 0 and np.abs(host(want)[1]).max() > 0
    assert np.array_equal(host(same), c.vis)
    assert max(figs.values()) < TOL, figs
    assert ctx.get_option("errors") == 0
    c.im.close()


@pytest.mark.parametrize("kind", ["simple", "w_cache"])
def test_a_non_finite_x_grids_and_predicts_nothing(ctx, kind):
    import torch
    c = spectral_case(ctx, kind, bad=((5, np.nan), (17, np.inf), (40, -np.inf)))
    flagged = ~torch.isfinite(c.dx)
    assert int(flagged.sum()) == 3
    x = torch.where(flagged, torch.zeros_like(c.dx), c.dx)
    vis = c.dvis.clone()
    vis[5] = complex(float("nan"), float("nan"))  # a flagged visibility is selected out, not multiplied by zero
    clean_vis = torch.where(flagged, torch.zeros_like(vis), vis)
    psfs = host(c.im.spectral_psfs())
    for s in range(2 * T - 1):
        want = host(c.im.cycle(torch.where(flagged, torch.zeros_like(x), x ** s).to(torch.complex128)))
        assert np.abs(psfs[s] - want).max() < TOL, s
    models = to_dev(np.random.default_rng(3).normal(size=(T, c.N, c.N)))
    vis_res = torch.empty_like(vis)
    got = host(c.im.mfs_cycle(vis, models, vis_res=vis_res))
    want, r = composed(c, clean_vis, models, x, flagged)
    assert np.isfinite(got).all() and rel(got, host(want)) < TOL
    gr = host(vis_res)
    assert np.isnan(gr[5]) and gr[17] == c.vis[17] and gr[40] == c.vis[40]  # they predict 0: r = vis
    ok = ~host(flagged)
    assert rel(gr[ok], host(r)[ok]) < TOL
    c.im.close()


def test_without_spectral_terms_the_calls_are_refused_and_with_them_nothing_else_changes(ctx):
    import torch
    import gridhip
    c = Case(ctx, "w_cache", THETA, LAM, 3000, 11)
    N, n = c.N, c.im.n
    stack = torch.zeros((T, N, N), dtype=torch.float64, device="cuda:0")
    for call in (lambda: c.im.spectral_psfs(), lambda: c.im.mfs_cycle(c.dvis, out=stack),
                 lambda: c.im.mfclean(stack), lambda: c.im.mfdeconvolve(c.dvis, 1, out=stack)):
        with pytest.raises(gridhip.GridHipError) as ei:
            call()
        assert ei.value.code == gridhip._lib.EINVAL
    torch.cuda.synchronize()
    assert not bool(stack.any())
    for bad_T in (0, 5):
        assert ctx._lib.gridhip_imager_set_spectral_dev(c.im._h, bad_T, None) == gridhip._lib.EINVAL
    # before set_spectral ...
    kw = dict(gain=0.2, threshold=0.0, niter=50, border=3, patch=0)
    psf0, pmax0 = host(c.im.psf).copy(), c.im.pmax
    cyc0 = host(c.im.cycle(c.dvis, c.dmodel)).copy()
    cl0 = [host(t).copy() for t in c.im.clean(to_dev(cyc0), **kw)]
    # ... and after it: the PSF's bits, pmax and - on the same image - clean's bits are what they were; a cycle agrees
    # as two cycles of one imager do; so does a fresh imager's
    c.im.set_spectral(to_dev(np.random.default_rng(1).choice(CHANNELS, n)), T)
    c.im.mfs_cycle(c.dvis, to_dev(np.random.default_rng(2).normal(size=(T, N, N))))
    c.im._psf = None
    assert np.array_equal(host(c.im.psf), psf0) and c.im.pmax == pmax0
    assert rel(host(c.im.cycle(c.dvis, c.dmodel)), cyc0) < 1e-12
    for a, b in zip(cl0, c.im.clean(to_dev(cyc0), **kw)):
        assert np.array_equal(a, host(b))
    fresh = Case(ctx, "w_cache", THETA, LAM, 3000, 11)
    assert rel(host(fresh.im.cycle(fresh.dvis, fresh.dmodel)), cyc0) < 1e-12
    assert rel(host(fresh.im.psf), psf0) < 1e-12
    # set_spectral again replaces the terms: more of them, then fewer
    c.im.set_spectral(to_dev(np.zeros(n)), 3)
    p3 = host(c.im.spectral_psfs())
    assert p3.shape == (5, N, N) and rel(p3[0], psf0) < TOL and not p3[1:].any()  # x = 0: the higher terms vanish
    c.im.set_spectral(to_dev(np.ones(n)), 1)
    assert host(c.im.spectral_psfs()).shape == (1, N, N)
    fresh.im.close()
    c.im.close()


def wide_band_sky(ctx):
    """a w_cache imager and the visibilities of three point sources with spectral slopes: predict(m0) + x predict(m1)"""
    import torch
    c = Case(ctx, "w_cache", THETA, LAM, 6000, 71)
    x = to_dev(np.random.default_rng(72).choice(CHANNELS, c.im.n))
    N = c.N
    cells = [(40, 50), (70, 30), (85, 90)]
    amp, alpha = [1.0, 0.7, 0.5], [-0.8, 0.4, -1.2]
    m0, m1 = np.zeros((N, N)), np.zeros((N, N))
    for (y, xx), a, al in zip(cells, amp, alpha):
        m0[y, xx], m1[y, xx] = a, a * al
    vis = (c.im.predict(to_dev(m0)) + x * c.im.predict(to_dev(m1))).contiguous()
    torch.cuda.synchronize()
    return c, x, vis, cells, alpha


def test_mfdeconvolve_is_the_loop_it_replaces(ctx):
    import torch
    c, x, vis, _, _ = wide_band_sky(ctx)
    c.im.set_spectral(x, T)
    N = c.N
    kw = dict(gain=0.2, threshold=0.0, niter=40, border=2, patch=0)
    models, images, stats = c.im.mfdeconvolve(vis, 3, **kw)
    m2 = torch.zeros((T, N, N), dtype=torch.float64, device="cuda:0")
    rows, first = [], None
    for cyc in range(3):
        img = c.im.mfs_cycle(vis, m2)
        if first is None:
            first = host(img).copy()
        _, _, s = c.im.mfclean(img, m2, **kw)
        rows.append(host(s))
    closing = host(c.im.mfs_cycle(vis, m2))
    gm, gi, gs = host(models), host(images), host(stats)
    mp, ip = np.abs(host(m2)).max(), np.abs(closing).max()
    em, ei = np.abs(gm - host(m2)).max() / mp, np.abs(gi - closing).max() / ip
    bits = np.array_equal(gm, host(m2)) and np.array_equal(gi, closing)
    print(f"models {em:.2e} images {ei:.2e} (bit for bit: {bits}); dirty peak {np.abs(first[0]).max():.4g}, closing "
          f"{np.abs(closing[0]).max():.4g}")
    assert mp > 0 and em < TOL and ei < TOL
    assert np.array_equal(np.flatnonzero(gm), np.flatnonzero(host(m2)))
    assert gs.shape == (3, 8) and np.array_equal(gs[:, [0, 2, 7]], np.array(rows)[:, [0, 2, 7]])
    assert np.abs(gs - np.array(rows)).max() / np.abs(first[0]).max() < TOL
    assert np.abs(closing[0]).max() < np.abs(first[0]).max()
    c.im.close()


def test_two_terms_clean_deeper_than_one_on_sources_with_a_spectral_slope(ctx):
    """End to end: after the same three major cycles the term-0 residual image of the two-term run is flatter than the
    single-term deconvolve's, whose model cannot absorb the x-dependent part.  The recovered slopes are printed beside the
    true ones and not asserted: their margin is not yet measured."""
    import torch
    c, x, vis, cells, alpha = wide_band_sky(ctx)
    c.im.set_spectral(x, T)
    kw = dict(gain=0.2, threshold=0.0, niter=60, border=2, patch=0)
    _, single, _ = c.im.deconvolve(vis, 3, **kw)
    models, images, stats = c.im.mfdeconvolve(vis, 3, **kw)
    torch.cuda.synchronize()
    rms1, rms2 = float(host(single).std()), float(host(images)[0].std())
    gm = host(models)
    got = [gm[1][y, xx] / gm[0][y, xx] if gm[0][y, xx] != 0 else float("nan") for y, xx in cells]
    print(f"term-0 residual rms: single term {rms1:.3e}, two terms {rms2:.3e}; alpha true {alpha}, recovered "
          f"{[round(float(g), 3) for g in got]}; iterations {host(stats)[:, 0]}")
    assert rms2 < rms1
    c.im.close()
