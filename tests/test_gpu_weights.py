"""Imaging weights on the GPU (gridhip_weights*, the weighted imager creations, Context.weights, Context.imager(weighting=)),
against the numpy restatement tests/weights_ref.py and against compositions of existing calls.

Bounds, each from its source and none from what the code gives:
  * wt_in NULL: the density is an integer count and its sums 64-bit integers, so uniform weights without a taper are the
    bits of doweight on ones (1.0 / count), the three counts of stats are exact and two runs give the same bits; weights,
    f^2 and the sums agree with the restatement within 1e-13 relative - a handful of roundings plus libm's exp and pow (the
    tests keep the taper's exponent <= 50, so that exp's argument error stays inside it);
  * with data weights the density is summed by fp64 atomics in the order they arrive: 1e-10 relative, the project's
    figure for such sums (at most 1000 visibilities per cell here);
  * an imager against the composition of existing calls: 1e-10 of the largest magnitude, as tests/test_gpu_imager.py."""
import ctypes as C

import numpy as np
import pytest

import weights_ref
from oracle import gridref_np as P
from test_gpu_imager import KO, host, imgfn_of, setup, to_dev

pytestmark = pytest.mark.gpu

MODES = ["natural", "uniform", "briggs"]
TIGHT, ATOMIC = 1e-13, 1e-10


def stream(n, lam, seed, span=0.55, nans=True, sigma=0.18):
    """u, v in wavelengths: a Gaussian core (many visibilities per cell) plus a uniform part beyond the grid's edge"""
    rng = np.random.default_rng(seed)
    u = np.where(rng.random(n) < 0.5, rng.normal(0, sigma, n), rng.uniform(-span, span, n)) * lam
    v = np.where(rng.random(n) < 0.5, rng.normal(0, sigma, n), rng.uniform(-span, span, n)) * lam
    if nans and n > 10:
        u[3], v[5], u[7], v[7] = np.nan, np.nan, np.nan, np.nan
    return u, v


def data_weights(n, seed, flagged=True):
    rng = np.random.default_rng(seed + 100)
    s = rng.uniform(0.25, 4.0, n)
    if flagged and n > 20:
        s[rng.random(n) < 0.1] = 0.0
        s[11], s[12], s[13] = -1.0, np.nan, 0.0
    return s


def taper_for(u, v):
    """the smallest sigma that keeps the exponent (u^2 + v^2) / (2 sigma^2) <= 50 over the stream"""
    r2 = np.nanmax(u * u + v * v)
    return float(np.sqrt(r2 / 100.0)) * 1.0001


def close(got, want, tol):
    """relative agreement, element by element; NaN only where NaN is wanted (a tapered NaN coordinate)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= tol * np.abs(want[ok])))


def check(what, w, st, ref, tol):
    rw, rst, _ = ref
    err = np.nanmax(np.abs(w - rw) / np.where(rw == 0, 1.0, np.abs(rw))) if len(rw) else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        serr = np.abs(st[:5] - rst[:5]) / np.abs(rst[:5])
    print(what, f"weights {err:.2e} stats {np.array2string(serr, precision=1)} counts {st[5:]} / {rst[5:]}")
    assert close(w, rw, tol), what
    assert np.array_equal(w == 0, rw == 0) and not np.signbit(w[rw == 0]).any(), what  # flagged: exactly +0.0
    assert close(st[:5], rst[:5], tol), (what, st, rst)
    assert np.array_equal(st[5:], rst[5:]), (what, st, rst)


# ---- bits and counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,lam", [(0.1, 640), (0.1, 490)])
def test_uniform_without_data_weights_is_doweight_bit_for_bit(ctx, theta, lam):
    for n in (1, 2, 5001, 20000):
        u, v = stream(n, lam, 3 + n, nans=n > 10)
        want = ctx.doweight(theta, lam, (u, v), np.ones(n, dtype=np.complex128))
        assert np.all(want.imag == 0)
        w, st = ctx.weights(theta, lam, (u, v, None), "uniform")
        assert np.array_equal(w, want.real), n
        wd, std = ctx.weights(theta, lam, (to_dev(u), to_dev(v)), "uniform")
        assert np.array_equal(host(wd), want.real) and np.array_equal(host(std), st, equal_nan=True), n
        N = ctx.image_size(theta, lam)
        ref = weights_ref.weights(N, lam, u, v, "uniform")
        assert np.array_equal(w, ref[0]) and np.array_equal(st[5:], ref[1][5:])
        if n > 10:
            assert st[7] >= 3 and st[5] + st[7] == n and st[6] == 0 and w[3] == 1.0


# ---- against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,lam", [(0.1, 640), (0.1, 490)])  # N = 64 and N = 49
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("given", [False, True])
def test_against_the_restatement(ctx, theta, lam, stride, given):
    N = ctx.image_size(theta, lam)
    for n in (0, 1, 7, 30001):
        u, v = stream(n, lam, 17 + n)
        s = data_weights(n, n) if given else None
        if n > 10:
            assert np.bincount(weights_ref.cells(N, lam, u, v)[weights_ref.cells(N, lam, u, v) >= 0]).max() <= 1000
        p = np.stack([u, v, np.zeros(n)], axis=1) if stride == 3 else (u, v, None)
        dp = to_dev(p) if stride == 3 else (to_dev(u), to_dev(v))
        for mode in MODES:
            for robust in ((-1.0, 0.5) if mode == "briggs" else (0.0,)):
                for sigma in ((0.0, taper_for(u, v)) if n > 1 else (0.0,)):
                    ref = weights_ref.weights(N, lam, u, v, mode, robust, sigma, s)
                    tol = ATOMIC if given else TIGHT
                    what = f"N={N} n={n} stride={stride} {mode} R={robust} sigma={sigma:.3g} given={given}"
                    w, st = ctx.weights(theta, lam, p, mode, robust, sigma, s)
                    check("host " + what, w, st, ref, tol)
                    wd, std = ctx.weights(theta, lam, dp, mode, robust, sigma, None if s is None else to_dev(s))
                    check("dev  " + what, host(wd), host(std), ref, tol)
                    if not given:  # integer sums, fixed-order partial sums: the forms and two runs give the same bits
                        assert np.array_equal(host(wd), w, equal_nan=True) and np.array_equal(host(std), st, equal_nan=True)
                        w2, st2 = ctx.weights(theta, lam, dp, mode, robust, sigma)
                        assert np.array_equal(host(w2), w, equal_nan=True) and np.array_equal(host(st2), st, equal_nan=True)
                    if mode == "natural" and sigma == 0.0 and st[5] > 0:
                        assert abs(st[3] - 1.0) <= tol
                    elif st[5] > 1:  # (>= 1 by Cauchy-Schwarz; equal weights give 1 up to the roundings of the sums)
                        assert st[3] >= 1.0 - tol


def test_in_place_and_unaligned(ctx):
    """wt_out == wt_in; and arrays that start 8 bytes off a 16-byte boundary take the one-by-one path with the same bits"""
    import torch
    theta, lam, n = 0.1, 640, 12345
    N = ctx.image_size(theta, lam)
    u, v = stream(n, lam, 23)
    s = data_weights(n, 5)
    for mode in MODES:
        ref = weights_ref.weights(N, lam, u, v, mode, 0.0, taper_for(u, v), s)
        buf = s.copy()
        w, st = ctx.weights(theta, lam, (u, v), mode, 0.0, taper_for(u, v), weights=buf, out=buf)
        assert w is buf
        check("in place, host " + mode, w, st, ref, ATOMIC)
        dbuf = to_dev(s)
        wd, std = ctx.weights(theta, lam, (to_dev(u), to_dev(v)), mode, 0.0, taper_for(u, v), weights=dbuf, out=dbuf)
        assert wd is dbuf
        check("in place, dev " + mode, host(wd), host(std), ref, ATOMIC)
    # off by 8 bytes: views of longer tensors
    big = [torch.zeros(n + 1, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    du, dv, dout = (b[1:] for b in big)
    du.copy_(to_dev(u)), dv.copy_(to_dev(v))
    assert du.data_ptr() % 16 == 8 and du.is_contiguous()
    for mode in MODES:
        a, sa = ctx.weights(theta, lam, (to_dev(u), to_dev(v)), mode, 0.5, taper_for(u, v))
        b, sb = ctx.weights(theta, lam, (du, dv), mode, 0.5, taper_for(u, v), out=dout)
        assert np.array_equal(host(a), host(b), equal_nan=True) and close(host(sb), host(sa), TIGHT)
        assert np.array_equal(host(sb)[5:], host(sa)[5:])


def test_robust_limits_and_noise_on_the_device(ctx):
    theta, lam, n = 0.1, 640, 40000
    u, v = stream(n, lam, 31, nans=False)
    du = (to_dev(u), to_dev(v))
    nat, snat = (host(x) for x in ctx.weights(theta, lam, du, "natural"))
    uni, suni = (host(x) for x in ctx.weights(theta, lam, du, "uniform"))
    hi, _ = (host(x) for x in ctx.weights(theta, lam, du, "briggs", robust=8.0))
    lo, slo = (host(x) for x in ctx.weights(theta, lam, du, "briggs", robust=-8.0))
    inside = weights_ref.cells(64, lam, u, v) >= 0
    assert np.abs(hi / nat - 1).max() < 1e-12
    ratio = (lo / uni)[inside]
    assert np.abs(ratio / ratio[0] - 1).max() < 1e-12 and abs(ratio[0] * slo[4] - 1) < 1e-12
    assert snat[3] == 1.0 and suni[3] > 1.0 and slo[3] > 1.0 and snat[4] == 0.0 and suni[4] == 0.0 and slo[4] > 0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import gridhip
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    theta, lam, n = 0.1, 640, 64
    u, v = stream(n, lam, 41, nans=False)
    s = np.ones(n)
    out = np.full(n, 7.0)
    st = np.full(8, 9.0)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    uv = np.concatenate([u, v])  # wt_out overlapping u or v

    def refused(fn, *args):
        assert fn(h, *args) == _lib.EINVAL, args
        assert np.all(out == 7.0) and np.all(st == 9.0) and np.all(s == 1.0)
    bad = [
        (theta, lam, -1, p(u), p(v), 1, p(s), 1, 0.0, 0.0, p(out), p(st)),
        (theta, lam, n, None, p(v), 1, p(s), 1, 0.0, 0.0, p(out), p(st)),
        (theta, lam, n, p(u), None, 1, p(s), 1, 0.0, 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 1, 0.0, 0.0, None, p(st)),
        (theta, lam, n, p(u), p(v), 0, p(s), 1, 0.0, 0.0, p(out), p(st)),
        (0.0, lam, n, p(u), p(v), 1, p(s), 1, 0.0, 0.0, p(out), p(st)),           # N = 0
        (theta, -lam, n, p(u), p(v), 1, p(s), 1, 0.0, 0.0, p(out), p(st)),        # N < 0
        (theta, lam, n, p(u), p(v), 1, p(s), 3, 0.0, 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), -1, 0.0, 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 2, float("nan"), 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 2, float("inf"), 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 0, float("-inf"), 0.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 1, 0.0, -1.0, p(out), p(st)),
        (theta, lam, n, p(u), p(v), 1, p(s), 1, 0.0, float("nan"), p(out), p(st)),
    ]
    for fn in (lib.gridhip_weights, lib.gridhip_weights_dev):
        for args in bad:
            refused(fn, *args)
        keep = uv.copy()
        pu, pv = C.c_void_p(uv.ctypes.data), C.c_void_p(uv.ctypes.data + 8 * n)
        for wo in (pu, pv, C.c_void_p(uv.ctypes.data + 8 * (n - 1)), C.c_void_p(uv.ctypes.data + 8)):
            assert fn(h, theta, lam, n, pu, pv, 1, p(s), 1, 0.0, 0.0, wo, p(st)) == _lib.EINVAL
        # a strided u spans 3 n doubles: an output inside that span overlaps it
        m = np.zeros((n, 3))
        pm = m.ctypes.data
        assert fn(h, theta, lam, n, C.c_void_p(pm), C.c_void_p(pm + 8), 3, None, 1, 0.0, 0.0, C.c_void_p(pm + 16 * n),
                  p(st)) == _lib.EINVAL
        assert np.array_equal(uv, keep) and np.all(m == 0) and np.all(st == 9.0)
    # the imager creations refuse a bad weighting before anything is made
    import torch
    duvw = tuple(to_dev(x) for x in (u, v, np.zeros(n)))
    hp = C.c_void_p(0xDEAD)
    for mode, robust, sigma in ((3, 0.0, 0.0), (-1, 0.0, 0.0), (2, float("nan"), 0.0), (1, 0.0, -1.0)):
        rc = lib.gridhip_imager_create_weighted_dev(h, 0, 0, 0, 0, 0, 0, None, theta, lam, n,
                                                    *(C.c_void_p(t.data_ptr()) for t in duvw), 1, mode, robust, sigma, None,
                                                    C.byref(hp))
        assert rc == _lib.EINVAL and not hp.value
        hp.value = 0xDEAD
    with pytest.raises(gridhip.GridHipError):
        ctx._call(_marshal_device(), "weights", theta, lam, n, duvw[0], duvw[1], 1, None, 5, 0.0, 0.0, duvw[2], None)
    torch.cuda.synchronize()
    assert np.all(host(duvw[2]) == 0)


def _marshal_device():
    from gridhip import _marshal
    return _marshal.device()


# ---- capture ---------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_to_the_same_result(ctx):
    import torch
    theta, lam, n = 0.1, 640, 50000
    u, v = stream(n, lam, 51)
    s = data_weights(n, 51)
    du, ds = (to_dev(u), to_dev(v)), to_dev(s)
    sig = taper_for(u, v)
    eager = [(host(a), host(b)) for a, b in (ctx.weights(theta, lam, du, "briggs", 0.5, sig),
                                             ctx.weights(theta, lam, du, "uniform", 0.0, 0.0, ds))]
    o1, o2 = (torch.zeros(n, dtype=torch.float64, device="cuda:0") for _ in range(2))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        ctx.weights(theta, lam, du, "briggs", 0.5, sig, out=o1)
        ctx.weights(theta, lam, du, "uniform", 0.0, 0.0, ds, out=o2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        _, s1 = ctx.weights(theta, lam, du, "briggs", 0.5, sig, out=o1)
        _, s2 = ctx.weights(theta, lam, du, "uniform", 0.0, 0.0, ds, out=o2)
    torch.cuda.synchronize()
    for _ in range(2):
        o1.fill_(7.0), o2.fill_(7.0), s1.fill_(7.0), s2.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(o1), eager[0][0], equal_nan=True) and np.array_equal(host(s1), eager[0][1])
        assert close(host(o2), eager[1][0], ATOMIC) and close(host(s2), eager[1][1], ATOMIC)
        assert np.array_equal(host(s2)[5:], eager[1][1][5:])


# ---- imagers ---------------------------------------------------------------------------------------------------------------
IMAGER_KINDS = ["simple", "w_cache", "aw"]


def imaging_call(ctx, kind, theta, lam, uvw, vis, aw):
    if kind == "simple":
        return ctx.simple_imaging(theta, lam, uvw, None, vis)
    if kind == "w_cache":
        return ctx.w_cache_imaging(KO, theta, lam, uvw, None, vis)
    return ctx.aw_imaging(theta, lam, aw[0], aw[1], aw[2], uvw, (aw[3], aw[4], None, None), vis)


def composed(ctx, kind, theta, lam, uvw, vis, aw, mode, robust, sigma, s):
    """mirror_uvw -> weights -> the imaging function of w vis1 and of w -> make_grid_hermitian -> ifft -> / max"""
    uvw1, vis1 = ctx.mirror_uvw(uvw, vis)
    w, st = ctx.weights(theta, lam, uvw1, mode, robust, sigma, s)
    img = ctx.ifft(ctx.make_grid_hermitian(imaging_call(ctx, kind, theta, lam, uvw1, w * vis1, aw))).real
    psf = ctx.ifft(ctx.make_grid_hermitian(imaging_call(ctx, kind, theta, lam, uvw1, w.astype(np.complex128), aw))).real
    pmax = psf.max()
    return img / pmax, psf / pmax, pmax, st


def make_imager(ctx, kind, theta, lam, uvw, aw, **kw):
    daw = None if aw is None else tuple(to_dev(x) for x in aw)
    a1, a2 = (daw[3], daw[4]) if daw is not None else (None, None)
    return ctx.imager(theta, lam, tuple(to_dev(x) for x in uvw), imgfn_of(kind, None, daw, KO), a1=a1, a2=a2, **kw)


@pytest.mark.parametrize("theta,lam", [(0.1, 640), (0.1, 490)])
@pytest.mark.parametrize("kind", IMAGER_KINDS)
def test_a_weighted_imager_is_the_composition_of_existing_calls(ctx, kind, theta, lam):
    n = 3000
    N, uvw, vis, _, _, aw = setup(kind, theta, lam, n, 61, bad_antennas=False)
    s = data_weights(n, 61, flagged=False)
    sigma = 0.4 * lam
    for mode, robust, sig, given in (("natural", 0.0, 0.0, False), ("uniform", 0.0, sigma, True),
                                     ("briggs", 0.0, 0.0, False), ("briggs", -0.5, sigma, True)):
        sw = s if given else None
        img, psf, pmax, st = composed(ctx, kind, theta, lam, uvw, vis, aw, mode, robust, sig, sw)
        im = make_imager(ctx, kind, theta, lam, uvw, aw, weighting=mode, robust=robust, taper=sig,
                         weights=None if sw is None else to_dev(sw))
        got = host(im.cycle(to_dev(vis)))
        figs = {"image": np.abs(got - img).max() / np.abs(img).max(),
                "psf": np.abs(host(im.psf) - psf).max() / np.abs(psf).max(), "pmax": abs(im.pmax - pmax) / abs(pmax)}
        print(kind, N, mode, robust, sig, given, figs)
        assert max(figs.values()) < 1e-10, figs
        assert close(host(im.weight_stats()), st, ATOMIC if given else TIGHT)
        im.close()


@pytest.mark.parametrize("kind", IMAGER_KINDS)
def test_the_default_creation_is_the_uniform_weighted_one(ctx, kind):
    theta, lam, n = 0.1, 640, 3000
    N, uvw, vis, model, _, aw = setup(kind, theta, lam, n, 67, bad_antennas=False)
    plain = make_imager(ctx, kind, theta, lam, uvw, aw)
    # (robust is not read by uniform weighting: a value other than 0 only routes the call to the weighted entry point)
    weighted = make_imager(ctx, kind, theta, lam, uvw, aw, weighting="uniform", robust=1.0)
    assert abs(plain.pmax - weighted.pmax) <= 1e-12 * abs(plain.pmax)  # (the PSF is gridded with fp64 atomics)
    assert np.array_equal(host(plain.weight_stats()), host(weighted.weight_stats()))
    assert np.abs(host(plain.psf) - host(weighted.psf)).max() <= 1e-10 * np.abs(host(plain.psf)).max()
    a = host(plain.cycle(to_dev(vis), to_dev(model)))
    b = host(weighted.cycle(to_dev(vis), to_dev(model)))
    assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()
    # and it is still do_imaging's: the stats are those of uniform weights on the mirrored stream
    uvw1, _ = ctx.mirror_uvw(uvw, vis)
    _, st = ctx.weights(theta, lam, uvw1, "uniform")
    assert np.array_equal(host(plain.weight_stats()), st)
    plain.close(), weighted.close()


@pytest.mark.parametrize("kind", IMAGER_KINDS)
@pytest.mark.parametrize("mode", ["uniform", "briggs"])
def test_flagged_visibilities_contribute_exactly_nothing(ctx, kind, mode):
    """20 % of the stream has weight 0 and a NaN (or Inf) visibility: the image is finite everywhere and equals the image
    of the stream with those visibilities removed"""
    theta, lam, n = 0.1, 640, 4000
    N, uvw, vis, model, _, aw = setup(kind, theta, lam, n, 71, bad_antennas=False)
    rng = np.random.default_rng(5)
    flagged = rng.random(n) < 0.2
    s = np.where(flagged, 0.0, rng.uniform(0.5, 2.0, n))
    s[np.flatnonzero(flagged)[:3]] = [-1.0, np.nan, 0.0]
    bad = vis.copy()
    bad[flagged] = np.nan + 1j * np.nan
    bad[np.flatnonzero(flagged)[5]] = np.inf
    keep = ~flagged
    im = make_imager(ctx, kind, theta, lam, uvw, aw, weighting=mode, robust=0.3, weights=to_dev(s))
    aw_k = None if aw is None else (aw[0], aw[1], aw[2], aw[3][keep], aw[4][keep])
    ref = make_imager(ctx, kind, theta, lam, tuple(x[keep] for x in uvw), aw_k, weighting=mode, robust=0.3,
                      weights=to_dev(s[keep]))
    st = host(im.weight_stats())
    assert st[6] == flagged.sum() and close(st[:6], host(ref.weight_stats())[:6], ATOMIC)
    for m in (None, to_dev(model)):
        vis_res = to_dev(np.zeros(n, dtype=np.complex128))
        got = host(im.cycle(to_dev(bad), m, vis_res=vis_res))
        want = host(ref.cycle(to_dev(vis[keep]), m))
        assert np.isfinite(got).all() and np.isfinite(host(im.psf)).all()
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
        assert not np.isfinite(host(vis_res)[flagged]).any() and np.isfinite(host(vis_res)[keep]).all()  # still vis - pred
    assert np.abs(host(im.psf) - host(ref.psf)).max() <= 1e-10 and abs(im.pmax - ref.pmax) <= 1e-10 * ref.pmax
    im.close(), ref.close()


def test_natural_weighting_gives_a_wider_beam_and_no_noise_penalty(ctx):
    """a centrally concentrated uv distribution: natural weighting keeps the core's weight and fits a larger beam than
    uniform weighting, whose noise ratio is above 1"""
    theta, lam, n = 0.1, 1280, 60000  # N = 128
    rng = np.random.default_rng(83)
    u, v = rng.normal(0, 0.08 * lam, n), rng.normal(0, 0.08 * lam, n)
    uvw = (u, v, np.zeros(n))
    nat = make_imager(ctx, "simple", theta, lam, uvw, None, weighting="natural")
    uni = make_imager(ctx, "simple", theta, lam, uvw, None)
    bn, bu = host(nat.beam()), host(uni.beam())
    sn, su = host(nat.weight_stats()), host(uni.weight_stats())
    print("bmaj natural", bn[3], "uniform", bu[3], "noise", sn[3], su[3])
    assert bn[7] == 1.0 and bu[7] == 1.0 and bn[3] > bu[3]
    assert abs(sn[3] - 1.0) <= TIGHT and su[3] > 1.0
    nat.close(), uni.close()


def test_deconvolve_and_restore_on_a_briggs_imager(ctx):
    import torch
    theta, lam, n = 0.1, 640, 20000
    N = 64
    rng = np.random.default_rng(89)
    u, v = rng.normal(0, 0.15 * lam, n), rng.normal(0, 0.15 * lam, n)
    uvw = (u, v, rng.uniform(-50, 50, n))
    s = rng.uniform(0.5, 2.0, n)
    im = make_imager(ctx, "simple", theta, lam, uvw, None, weighting="briggs", robust=0.0, weights=to_dev(s))
    sky = np.zeros((N, N))
    spots = [(20, 41), (40, 25)]
    sky[spots[0]], sky[spots[1]] = 1.0, 0.7
    vis = im.predict(to_dev(sky))
    model, image, stats = im.deconvolve(vis, 3, gain=0.2, niter=60, border=2)
    restored, beam = im.restore(model, image, support=6)
    torch.cuda.synchronize()
    m, r = host(model), host(restored)
    assert host(beam)[7] == 1.0 and np.isfinite(r).all()
    top = sorted(np.argsort(m.ravel())[-2:].tolist())
    assert top == sorted(y * N + x for y, x in spots), (top, spots)
    assert np.unravel_index(np.argmax(r), r.shape) == spots[0]
    im.close()
