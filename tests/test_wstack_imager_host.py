"""The imager of the w-stacking kind (include/gridhip.h, "imagers", kind 4), the checks that need no GPU: the binding
hands ("wstack", kernops) to gridhip_imager_create_dev as kind 4 under wstack_options' rules, a NULL context is refused
for the kind, and the numpy restatement the GPU tests compare with (tests/wstack_imager_ref.py) gives, for a cycle
without a model, what the restatement of gridhip_do_imaging_wstack gives."""
import ctypes as C

import numpy as np
import pytest

import wstack_imager_ref as WI
import wstack_ref as W


def test_the_binding_maps_wstack_to_kind_4():
    from gridhip._marshal import HOST, imaging_function, wstack_options
    ko = dict(wstep=100, planes=8, qpx=4, npixFF=16, npixKern=7)
    assert imaging_function(HOST, ("wstack", ko)) == (4, 100, 4, 16, 7, 8, None)
    # (kind, wstep, Q, npixFF, gh = npixKern, gw = planes, kv): the same numbers as wstack_options', in the imager's order
    wstep, M, Q, ff, S = wstack_options(ko)
    assert imaging_function(HOST, ("wstack", ko)) == (4, wstep, Q, ff, S, M, None)
    # no wstep, or 0: 2000, the one rule
    for k in (dict(ko, wstep=0), {x: y for x, y in ko.items() if x != "wstep"}):
        assert imaging_function(HOST, ("wstack", k))[:2] == (4, 2000)
    # the other kinds are what they were
    assert imaging_function(HOST, ("simple",)) == (0, 0, 0, 0, 0, 0, None)
    assert imaging_function(HOST, ("w_cache", dict(qpx=2, npixFF=16, npixKern=9)))[:6] == (2, 2000, 2, 16, 9, 9)
    with pytest.raises(ValueError, match="unknown imaging function"):
        imaging_function(HOST, ("nothing",))


@pytest.mark.parametrize("bad", [dict(planes=0), dict(planes=-2), dict(wstep=-1), dict(npixKern=17), dict(qpx=0),
                                 dict(npixFF=5, npixKern=5)])
def test_wstack_options_refusals_pass_through(bad):
    from gridhip._marshal import HOST, imaging_function
    ko = dict(wstep=100, planes=8, qpx=4, npixFF=16, npixKern=7)
    with pytest.raises(ValueError, match="wstack:"):
        imaging_function(HOST, ("wstack", dict(ko, **bad)))
    with pytest.raises(KeyError):
        imaging_function(HOST, ("wstack", {k: v for k, v in ko.items() if k != "planes"}))


def test_a_null_context_is_refused_for_kind_4():
    from gridhip import _lib
    lib = _lib.load()
    x = (C.c_double * 8)()
    p = C.cast(x, C.c_void_p)
    for kind in (4, 3, 5):
        h = C.c_void_p(0x1234)  # a refused creation hands back NULL, not what was there
        assert lib.gridhip_imager_create_dev(None, kind, 100, 4, 16, 7, 8, None, 0.1, 640, 1, p, p, p, 1,
                                             C.byref(h)) == _lib.EINVAL
        assert not h.value
        h = C.c_void_p(0x1234)
        assert lib.gridhip_imager_create_weighted_dev(None, kind, 100, 4, 16, 7, 8, None, 0.1, 640, 1, p, p, p, 1, 2, 0.0,
                                                      0.0, None, C.byref(h)) == _lib.EINVAL
        assert not h.value


def test_a_cycle_without_a_model_is_do_imaging():
    """N = 48; u, v of both signs, so that the mirror acts; w over several layers"""
    theta, lam, wstep, M, S, ff, q = 0.15, 320, 100, 3, 7, 16, 2
    rng = np.random.default_rng(3)
    n = 400
    u, v = rng.uniform(-0.4 * lam, 0.4 * lam, n), rng.uniform(-0.4 * lam, 0.4 * lam, n)
    w = rng.uniform(-700, 700, n)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    img, psf, pmax = W.do_imaging(theta, lam, u, v, w, vis, wstep, M, q, ff, S)
    im = WI.StackImager(theta, lam, u, v, w, wstep, M, q, ff, S)
    assert im.N == 48 and im.neg.any() and not im.neg.all()
    assert im.gather.lay["L"] > 1 and not np.array_equal(im.gather.lay["layer"], im.scatter.lay["layer"])
    got, res = im.cycle(vis)
    # the same operations in the same order: equal to rounding
    tol = 1e-13
    assert np.abs(got - img).max() <= tol * np.abs(img).max()
    assert np.abs(im.psf - psf).max() <= tol * np.abs(psf).max() and abs(im.pmax - pmax) <= tol * pmax
    assert np.array_equal(res, vis)
    # with a model: do_imaging of the residual, and the prediction is the un-mirrored stream's
    model = rng.normal(size=(48, 48))
    pred = W.predict(theta, lam, u, v, w, model, wstep, M, q, ff, S)
    got, res = im.cycle(vis, model)
    img2, _, _ = W.do_imaging(theta, lam, u, v, w, vis - pred, wstep, M, q, ff, S)
    assert np.array_equal(res, vis - pred) and np.abs(got - img2).max() <= tol * np.abs(img2).max()
    # a weight that is not > 0 selects the sample out even under a NaN
    wt = im.wt.copy()
    wt[7] = 0.0
    bad = vis.copy()
    bad[7] = np.nan
    a = WI.StackImager(theta, lam, u, v, w, wstep, M, q, ff, S, weights=wt)
    keep = np.arange(n) != 7
    b = WI.StackImager(theta, lam, u[keep], v[keep], w[keep], wstep, M, q, ff, S, weights=wt[keep])
    ga, gb = a.cycle(bad)[0], b.cycle(vis[keep])[0]
    assert np.isfinite(ga).all() and np.abs(ga - gb).max() <= tol * np.abs(gb).max()
