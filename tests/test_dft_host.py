"""Direct-Fourier prediction without a GPU: the ABI is there, the header states the semantics, and the numpy reference
(tests/dft_ref.py) has the convention of the library's own transform."""
import os
import re

import numpy as np
import pytest

import dft_ref
import gaincal_ref
from conftest import ROOT
from oracle import gridref_np as P

HEADER = os.path.join(ROOT, "include", "gridhip.h")


def test_version_signatures_and_header():
    from gridhip import _lib
    raw = open(HEADER).read()
    assert _lib.load().gridhip_version() >= 220
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", raw).group(1)) >= 220
    assert int(re.search(r"#define GRIDHIP_COMP_DOUBLES (\d+)", raw).group(1)) == dft_ref.COMP_DOUBLES == 10
    lib = _lib.load()
    for name in ("gridhip_dft_predict", "gridhip_dft_predict_dev", "gridhip_components_from_image",
                 "gridhip_components_from_image_dev"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    text = " ".join(raw.split())
    assert "{ l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0 }" in text  # the layout
    assert "the phase is -2 pi (u l + v m + w (n - 1))" in text  # the sign
    assert "DETERMINISM. For a given (n, C, options) the result has the same bits on every run" in text
    assert "no atomics in the sum" in text and '"dft_slices"' in text


def test_python_surface():
    import gridhip
    assert callable(gridhip.Context.dft_predict) and callable(gridhip.Context.components_from_image)
    c = gridhip.components([0.1, -0.2], [0.0, 0.3], [1.0, 2.0], spectral=[[0.5], [-0.5]], fwhm=[[2e-4, 1e-4], [0, 0]],
                           pa=[0.3, 0.0])
    want = np.array([[0.1, 0.0, 1.0, 0.5, 0, 0, 2e-4, 1e-4, 0.3, 0], [-0.2, 0.3, 2.0, -0.5, 0, 0, 0, 0, 0, 0]])
    assert c.dtype == np.float64 and np.array_equal(c, want)
    with pytest.raises(ValueError):
        gridhip.components([0.1], [0.0], [1.0], spectral=[[1, 2, 3, 4]])


@pytest.mark.parametrize("N", [16, 15])
def test_reference_has_the_transforms_convention(N):
    """the DFT of a one-pixel model at the integer cells is fft_c(model): the pixel rule and the sign"""
    theta = 0.05
    model = np.zeros((N, N))
    model[N // 2 + 3, N // 2 - 5] = 1.5
    F = P.fft_c(model.astype(np.complex128))
    comps = dft_ref.components_from_image(theta, model)
    assert comps.shape == (1, 10) and comps[0, 2] == 1.5
    iy, ix = np.mgrid[0:N, 0:N]
    u, v = ((ix - N // 2) / theta).ravel(), ((iy - N // 2) / theta).ravel()
    got, st = dft_ref.dft_predict(comps, u, v)
    assert np.abs(got - F.ravel()).max() <= 1e-13 and list(st) == [1, 0, 0]


def test_reference_rules():
    """skipped components, non-finite visibilities, count, the residual and the spectral terms, on cases worked by hand"""
    c = np.zeros((5, 10))
    c[:, 2] = 1.0
    c[1, 0] = np.nan           # a NaN field
    c[2, 0] = c[2, 1] = 0.8    # r2 > 1
    c[3, 6:8] = 1e-4, 2e-4     # bmaj < bmin
    c[4, 6:8] = 1e-4, -1e-4    # a negative axis
    assert list(dft_ref.skipped(c, 1)) == [False, True, True, True, True]
    u, v = np.array([10.0, np.inf, 3.0]), np.array([0.0, 1.0, np.nan])
    out, st = dft_ref.dft_predict(c, u, v, vis_sub=np.full(3, 2 + 1j))
    assert list(st) == [1, 4, 2] and np.array_equal(out, [1 + 1j, 2 + 1j, 2 + 1j])
    out, st = dft_ref.dft_predict(c, u[:1], v[:1], count=-3)
    assert list(st) == [0, 0, 0] and out[0] == 0
    c = np.zeros((1, 10))
    c[0, 2:6] = 1, 2, 3, 4
    x = np.array([0.5])
    assert dft_ref.dft_predict(c, [0.0], [0.0], x=x, T=4)[0][0] == 1 + 0.5 * (2 + 0.5 * (3 + 0.5 * 4))
    assert dft_ref.dft_predict(c, [0.0], [0.0], x=x, T=2)[0][0] == 2.0 and dft_ref.dft_predict(c, [0.0], [0.0], T=4)[0][0] == 1.0
    # a Gaussian along m (bpa = 0) falls off with v, at the FWHM's rate
    c = np.zeros((1, 10))
    c[0, 2], c[0, 6] = 1.0, 1e-3
    v = 2 * np.log(2) / (np.pi * 1e-3)  # where E = 1/2
    assert abs(dft_ref.dft_predict(c, [0.0, v], [v, 0.0])[0] - [0.5, 1.0]).max() < 1e-15


def test_selfcal_case_on_the_references_alone():
    """the end-to-end case of test_gpu_dft.py, numpy only: the solve against the exact model reaches a chi^2 of 4.168e-11,
    against the nearest-cell prediction of the pixelised sources 341.1 - the ratio the GPU test asserts"""
    theta, lam, N, A, u, v, a1, a2, comps, model, gt = dft_ref.selfcal_observation()
    exact = dft_ref.dft_predict(comps, u, v)[0]
    vis = gaincal_ref.apply_gains(gt, exact, a1, a2, inverse=False)[0]
    F = P.fft_c(model.astype(np.complex128))
    x = N // 2 + np.floor(0.5 + N * (u / lam)).astype(np.int64)
    y = N // 2 + np.floor(0.5 + N * (v / lam)).astype(np.int64)
    assert x.min() >= 0 and y.min() >= 0 and x.max() < N and y.max() < N
    gA, sA = gaincal_ref.gaincal(vis, exact, a1, a2, A, **dft_ref.SELFCAL_SOLVE)
    gB, sB = gaincal_ref.gaincal(vis, F[y, x], a1, a2, A, **dft_ref.SELFCAL_SOLVE)
    print(f"chi2 exact {sA[2]:.4e} pixelised {sB[2]:.4e} ratio {sA[2] / sB[2]:.4e}")
    assert sA[2] / sB[2] <= dft_ref.SELFCAL_RATIO
    assert np.abs(gA - gt * np.exp(-1j * np.angle(gt[:, :1]))).max() < 1e-6
