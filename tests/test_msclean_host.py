"""CPU checks of multi-scale CLEAN's definition and binding: the numpy restatement (tests/msclean_ref.py) on a case worked
by hand, its agreement with the Hogbom restatement for the delta scale alone, and what Context.msclean hands to the C
ABI (against the recording library of tests/test_binding_marshalling.py)."""
import ctypes as C

import numpy as np
import pytest

import clean_ref
import msclean_ref
import restore_ref
from test_binding_marshalling import HANDLE, Arr, Out, Recorder, Same, f64


def test_scale_kernel_by_hand():
    """a = 2: R = 1, t = 1 - r^2 / 4 = 1 at the centre, 3/4 on the edges, 1/2 on the corners; the sum is 6 - all exact"""
    m = msclean_ref.scale_kernel(2.0)
    want = np.array([[0.5, 0.75, 0.5], [0.75, 1.0, 0.75], [0.5, 0.75, 0.5]]) / 6.0
    assert np.array_equal(m, want)
    assert np.array_equal(msclean_ref.scale_kernel(0.0), [[1.0]])
    assert np.array_equal(msclean_ref.scale_kernel(1.0), [[1.0]])  # R = 0: the support is the centre alone
    m = msclean_ref.scale_kernel(1.5)  # R = 1: the corners are max(0, 1 - 2 / 2.25), the edges 1 - 1 / 2.25
    e, k = 1.0 - 1.0 / 2.25, 1.0 - 2.0 / 2.25
    total = ((k + e) + k) + ((e + 1.0) + e) + ((k + e) + k)  # rows in dx order, then in dy order
    assert np.array_equal(m, np.array([[k, e, k], [e, 1.0, e], [k, e, k]]) / total)


def test_one_component_by_hand():
    """N = 8, the PSF a delta, scales [0, 2], the residual m_2 placed at (4, 3) times 12.  All values are small dyadic
    multiples of 1/6 or 1/36, so the restatement can be followed with a pencil:
      P_1 = m, P_11 = m (*) m, q_1 = sum of m^2 = (4 * .25 + 4 * .5625 + 1) / 36 = 4.25 / 36
      R_1 = 12 (m (*) m) shifted: its peak is at (4, 3), 12 q_1
      scale 0 offers |1 * 12 / 6|= 2 (the centre of 12 m), scale 1 offers b_1 * 12: scale 1 wins for b_1 > 1 / 6
      f = 1 * (12 q_1 / q_1) = 12 at gain 1: the model receives 12 m, and the residual loses 12 P_01 = 12 m - everything."""
    N = 8
    psf = np.zeros((N, N))
    psf[4, 4] = 1.0
    m = msclean_ref.scale_kernel(2.0)
    res = np.zeros((N, N))
    res[3:6, 2:5] = 12.0 * m
    start = res.copy()
    model, trace = np.zeros((N, N)), []
    st = msclean_ref.msclean(psf, res, model, [0.0, 2.0], [1.0, 0.4], 1.0, 0.0, 1, trace=trace)
    assert [(s, k) for s, k, _ in trace] == [(1, 4 * N + 3)]
    assert st[0] == 1 and st[3] == 1 and st[6:].tolist() == [0, 1, 0, 0, 0, 0]
    assert abs(st[4] - 12.0) < 1e-14
    assert np.abs(model - start).max() < 1e-14 and np.abs(res).max() < 1e-14
    # with a bias below 1 / 6 the delta wins: a Hogbom component of 12 / 6 at the centre
    res2, model2, trace2 = start.copy(), np.zeros((N, N)), []
    msclean_ref.msclean(psf, res2, model2, [0.0, 2.0], [1.0, 0.1], 1.0, 0.0, 1, trace=trace2)
    assert [(s, k) for s, k, _ in trace2] == [(0, 4 * N + 3)]
    assert model2[4, 3] == 2.0 and np.count_nonzero(model2) == 1 and res2[4, 3] == 0.0


@pytest.mark.parametrize("N", [96, 97])
def test_the_delta_scale_alone_is_hogbom_bit_for_bit(N):
    psf = restore_ref.smooth_psf(N, 11, 0.5)
    img, _ = msclean_ref.extended_sky(psf, 12)
    kw = dict(gain=0.2, threshold=0.0, niter=60)
    for border, patch in ((0, 0), (N // 8, 20)):
        r1, m1 = img.copy(), np.zeros_like(img)
        s1 = clean_ref.clean(psf, r1, m1, border=border, patch=patch, **kw)
        r2, m2 = img.copy(), np.zeros_like(img)
        s2 = msclean_ref.msclean(psf, r2, m2, [0.0], [1.0], border=border, patch=patch, **kw)
        assert np.array_equal(r1, r2) and np.array_equal(m1, m2)
        assert s2[0] == s1[0] == 60 and s2[1] == s1[1] and s2[2] == s1[2] and s2[4] == s1[3] and s2[6] == 60


def test_multi_scale_recovers_extended_flux():
    """the reason for the feature, on the restatement: at equal niter and gain the multi-scale residual is far flatter"""
    N = 96
    psf = restore_ref.smooth_psf(N, 11, 0.5)
    img, flux = msclean_ref.extended_sky(psf, 12)
    r1, m1 = img.copy(), np.zeros_like(img)
    clean_ref.clean(psf, r1, m1, 0.2, 0.0, 150)
    scales = [0.0, 4.0, 10.0]
    r2, m2 = img.copy(), np.zeros_like(img)
    st = msclean_ref.msclean(psf, r2, m2, scales, msclean_ref.default_bias(scales), 0.2, 0.0, 150)
    print(f"flux {flux:.1f}: hogbom {m1.sum():.1f} rms {r1.std():.4f}; multi-scale {m2.sum():.1f} rms {r2.std():.4f}; "
          f"per scale {st[6:9]}")
    assert r2.std() < 0.5 * r1.std() and np.count_nonzero(st[6:9]) >= 2


class HostArr:
    """a POINTER(c_double) argument addressing these host values (msclean's scales and bias, in every form)"""

    def __init__(self, values):
        self.want = np.array(values, dtype=f64)

    def check(self, arg, where):
        assert isinstance(arg, C.POINTER(C.c_double)), f"{where}: {type(arg)}"
        got = np.array([arg[i] for i in range(self.want.size)])
        assert np.array_equal(got, self.want), f"{where}: {got} != {self.want}"


def test_msclean_marshalling():
    import gridhip
    rec = Recorder()
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = rec, HANDLE, 0
    N = 6
    img = np.arange(N * N, dtype=f64).reshape(N, N)
    psf32 = np.arange(N * N, dtype=np.float32).reshape(N, N)  # converted; the image and the model go as they are
    model = np.zeros((N, N))
    o = Out(f64, 12)
    try:
        rec.expect("gridhip_msclean", HANDLE, (N, Arr(psf32, f64), Same(img), Same(model), 3, HostArr([0, 4, 10]),
                                               HostArr([1.0, 1 - 0.6 * 0.4, 0.4]), 0.25, 0.5, 7, 1, 2, o))
        m, r, s = ctx.msclean(img, psf32, [0, 4, 10], gain=0.25, threshold=0.5, niter=7, border=1, patch=2, model=model)
        assert m is model and r is img and o.returned(s, (12,))
        # an explicit bias of another dtype, and a new model of zeros
        rec.expect("gridhip_msclean", HANDLE, (N, Arr(psf32, f64), Same(img), Arr(np.zeros(N * N), f64), 2,
                                               HostArr([0, 2.5]), HostArr([1, 3]), 0.1, 0.0, 100, 0, 0, o))
        ctx.msclean(img, psf32, np.array([0, 2.5], dtype=np.float32), bias=[1, 3])
        # the delta alone: the default bias is 1
        rec.expect("gridhip_msclean", HANDLE, (N, Arr(psf32, f64), Same(img), Same(model), 1, HostArr([0]), HostArr([1]),
                                               0.1, 0.0, 100, 0, 0, o))
        ctx.msclean(img, psf32, [0], model=model)
        assert rec.calls == ["gridhip_msclean"] * 3
        for bad in (lambda: ctx.msclean(img, psf32, [0, 4], bias=[1.0]), lambda: ctx.msclean(img, psf32, []),
                    lambda: ctx.msclean(img.astype(np.float32), psf32, [0]), lambda: ctx.msclean(img, psf32[:, :3], [0])):
            with pytest.raises(ValueError):
                bad()
        assert rec.calls == ["gridhip_msclean"] * 3
    finally:
        ctx._h = None
