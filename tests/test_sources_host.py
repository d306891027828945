"""Source finding (gridhip_find_sources*), the checks that need no GPU: the library, the header, the ctypes table and the
bindings carry every new name; NULL handles and every argument the header refuses are refused with nothing touched; the
Python methods hand the ABI the right pointers and order (against a recording library); and the restatement the GPU tests
compare with (tests/sources_ref.py) is right on cases computed by hand and recovers the flux, position and intrinsic shape
of analytic Gaussians."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import sources_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Same
from test_clean_host import SameT, rig, tensor_returned, torch_rig  # noqa: F401  (fixtures)

NAMES = ["gridhip_find_sources", "gridhip_find_sources_dev", "gridhip_imager_find_sources_dev"]
f64, i64 = np.float64, np.int64
nan, inf = float("nan"), float("inf")


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_library_header_and_tables_carry_the_names():
    from gridhip import _lib
    text = open(os.path.join(ROOT, "include", "gridhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["gridhip_find_sources"] == _lib.SIGNATURES["gridhip_find_sources_dev"]
    assert "source finding" in text and re.search(r"#define GRIDHIP_SRC_DOUBLES 16\b", text)
    assert _lib.load().gridhip_version() >= 250
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", text).group(1)) >= 250


def test_bindings_carry_the_names():
    import gridhip
    for cls in (gridhip.Context, gridhip.Imager):
        assert callable(cls.find_sources)
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    assert "findSourcesIO" in head and re.search(r"^findSourcesIO ::", hs, flags=re.M)
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert "gridhip_find_sources(" in hpp


class Call:
    """one call of the three forms on host arrays that must come back untouched; N = image_size(0.1, 80) = 8"""
    ORDER = ("theta", "lam", "image", "border", "thr_hi", "thr_lo", "nsigma_hi", "nsigma_lo", "noise", "peak_frac", "min_cells",
             "beam", "correct", "max_c", "comps", "info", "count", "stats")

    def __init__(self, N=8, max_c=4):
        self.image, self.noise = np.full(N * N, 1.5), np.full(1, 9.0)
        self.beam = np.array([0.3, 0.0, 0.3, 0.0, 0.0, 0.0, 8.0, 1.0])
        self.comps, self.info = np.full(max_c * 10, 3.0), np.full(max_c * 16, 4.0)
        self.count, self.stats = np.full(1, 6, dtype=i64), np.full(8, 7.0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self.kw = dict(theta=0.1, lam=10 * N, image=p(self.image), border=0, thr_hi=1.0, thr_lo=0.5, nsigma_hi=5.0,
                       nsigma_lo=2.5, noise=p(self.noise), peak_frac=0.1, min_cells=1, beam=p(self.beam), correct=1,
                       max_c=max_c, comps=p(self.comps), info=p(self.info), count=p(self.count), stats=p(self.stats))

    def args(self, **change):
        kw = dict(self.kw, **change)
        return [kw[k] for k in self.ORDER]

    def untouched(self):
        return (np.all(self.image == 1.5) and self.noise[0] == 9.0 and self.beam[0] == 0.3 and np.all(self.comps == 3.0)
                and np.all(self.info == 4.0) and self.count[0] == 6 and np.all(self.stats == 7.0))


# every argument GRIDHIP_EINVAL refuses: auto-masking's (tests/test_automask_host.py) without absolute, mask and grow, and
# the call's own.  N = 8: border 4 makes 2 * border >= N.  lam 0, -80: an image size of 0, -8
EINVAL_CASES = [
    dict(thr_hi=0.25), dict(nsigma_lo=6.0),
    dict(thr_hi=-1.0, thr_lo=-2.0), dict(thr_lo=-0.5), dict(thr_hi=inf), dict(thr_hi=nan), dict(thr_lo=nan),
    dict(nsigma_hi=inf), dict(nsigma_hi=nan), dict(nsigma_lo=-1.0), dict(nsigma_lo=nan),
    dict(peak_frac=1.0), dict(peak_frac=-0.1), dict(peak_frac=nan),
    dict(noise=None),
    dict(min_cells=0), dict(min_cells=-3),
    dict(image=None), dict(count=None), dict(stats=None), dict(comps=None),
    dict(lam=0), dict(lam=-80), dict(border=4), dict(border=5), dict(border=-1),
    dict(max_c=-1), dict(correct=2), dict(correct=-1),
]


def test_null_handles_are_refused_and_nothing_is_touched():
    """A context cannot be made without a GPU, so what a host can see of the argument rules is this: whatever else is
    wrong with a call, a NULL handle is refused first and nothing is read or written.  The rules themselves are checked
    with a context in tests/test_gpu_sources.py::test_refusals, over the same list."""
    from gridhip import _lib
    lib = _lib.load()
    c = Call()
    for change in [{}] + EINVAL_CASES + [dict(lam=463410)]:
        a = c.args(**change)
        assert lib.gridhip_find_sources(None, *a) == _lib.EINVAL, change
        assert lib.gridhip_find_sources_dev(None, *a) == _lib.EINVAL, change
        assert lib.gridhip_imager_find_sources_dev(None, *a[2:]) == _lib.EINVAL, change
    assert c.untouched()


# ---- what the Python methods hand to the ABI ------------------------------------------------------------------------------
def test_context_find_sources_host_form(rig):
    ctx, rec, run = rig
    N = 6
    theta, lam = 0.1, 60
    image = np.arange(N * N, dtype=f64).reshape(N, N)
    beam = np.arange(8, dtype=f64)
    oc, oi, on, os_ = Out(f64, 3 * 10), Out(f64, 3 * 16), Out(i64, 1), Out(f64, 8)
    comps, count, info, stats = run(
        lambda: ctx.find_sources(theta, lam, image, beam, 0.125, border=1, thr=(2, 1), nsigma=(6, 3), peak_frac=0.25,
                                 min_cells=4, correct=False, max_sources=3),
        "gridhip_find_sources", theta, lam, Same(image), 1, 2.0, 1.0, 6.0, 3.0, Arr([0.125], f64), 0.25, 4, Same(beam), 0, 3,
        oc, oi, on, os_)
    assert oc.returned(comps, (3, 10)) and oi.returned(info, (3, 16)) and os_.returned(stats, (8,))
    assert type(count) is int and count == 1
    # defaults: no beam, the noise one element of a stats array by its own address, 1024 rows, correct; out is written in place
    st8 = np.arange(8, dtype=f64)
    out = np.zeros((1024, 10))
    comps, count, info, stats = run(lambda: ctx.find_sources(theta, lam, image, noise=st8[3:4], out=out),
                                    "gridhip_find_sources", theta, lam, Same(image), 0, 0.0, 0.0, 5.0, 2.5, Same(st8, 24), 0.0, 1,
                                    None, 1, 1024, Same(out), Out(f64, 1024 * 16), Out(i64, 1), Out(f64, 8))
    assert comps is out and info.shape == (1024, 16)
    # fixed levels need no noise; info=False passes NULL and returns None; max_sources=0; a float32 image is converted
    comps, count, info, stats = run(
        lambda: ctx.find_sources(theta, lam, image.astype(np.float32), thr=1.5, nsigma=0, max_sources=0, info=False),
        "gridhip_find_sources", theta, lam, Arr(image, f64), 0, 1.5, 1.5, 0.0, 0.0, None, 0.0, 1, None, 1, 0, Out(f64, 0), None,
        Out(i64, 1), Out(f64, 8))
    assert info is None and comps.shape == (0, 10)
    bad = [
        lambda: ctx.find_sources(theta, lam, image),                                  # nsigma > 0 and no noise
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, nsigma=(2, 3)),        # lo above hi
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, thr=(-1, -1)),
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, peak_frac=1.0),
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, min_cells=0),
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, max_sources=-1),
        lambda: ctx.find_sources(theta, lam, image, beam=np.zeros(7), noise=1.0),
        lambda: ctx.find_sources(theta, lam, image, beam=[0.0] * 8, noise=1.0),       # not an array of the call's kind
        lambda: ctx.find_sources(theta, lam, image, noise=np.zeros(2)),
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, out=np.zeros((5, 10)), max_sources=4),
        lambda: ctx.find_sources(theta, lam, image, noise=1.0, out=np.zeros((4, 10), dtype=np.float32), max_sources=4),
        lambda: ctx.find_sources(theta, 70, image, noise=1.0),                        # image_size(0.1, 70) = 7
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert rec.calls.count("gridhip_find_sources") == 3


def test_device_and_imager_forms(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, h = im.N, im._h
    theta, lam = 0.1, 10 * N
    image = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    beam = torch.arange(8, dtype=torch.float64)
    sig = torch.arange(8, dtype=torch.float64)
    oc, oi, on, os_ = Out(f64, 3 * 10), Out(f64, 3 * 16), Out(i64, 1), Out(f64, 8)
    comps, count, info, stats = run(
        lambda: ctx.find_sources(theta, lam, image, beam, sig[3:4], 1, (2, 1), (6, 3), 0.25, 4, False, 3),
        "gridhip_find_sources_dev", theta, lam, SameT(image), 1, 2.0, 1.0, 6.0, 3.0, SameT(sig[3:4]), 0.25, 4, SameT(beam), 0, 3,
        oc, oi, on, os_)
    assert tensor_returned(oc, comps, (3, 10)) and tensor_returned(oi, info, (3, 16)) and tensor_returned(os_, stats, (8,))
    assert isinstance(count, torch.Tensor) and count.dtype == torch.int64 and tuple(count.shape) == (1,) and int(count[0]) == 1
    assert bound == [ctx]
    oc, oi, on, os_ = Out(f64, 2 * 10), Out(f64, 2 * 16), Out(i64, 1), Out(f64, 8)
    comps, count, info, stats = run(
        lambda: im.find_sources(image, beam, sig[3:4], border=1, thr=(2, 1), nsigma=(6, 3), peak_frac=0.25, min_cells=4,
                                max_sources=2),
        "gridhip_imager_find_sources_dev", SameT(image), 1, 2.0, 1.0, 6.0, 3.0, SameT(sig[3:4]), 0.25, 4, SameT(beam), 1, 2,
        oc, oi, on, os_, handle=h)
    assert tensor_returned(oc, comps, (2, 10)) and tensor_returned(oi, info, (2, 16)) and tensor_returned(os_, stats, (8,))
    assert isinstance(count, torch.Tensor) and int(count[0]) == 1
    out = torch.zeros((4, 10), dtype=torch.float64)
    comps, count, info, stats = run(lambda: im.find_sources(image, nsigma=0, thr=(3, 1), max_sources=4, out=out, info=False),
                                    "gridhip_imager_find_sources_dev", SameT(image), 0, 3.0, 1.0, 0.0, 0.0, None, 0.0, 1, None,
                                    1, 4, SameT(out), None, Out(i64, 1), Out(f64, 8), handle=h)
    assert comps is out and info is None
    before = len(rec.calls)
    bad = [
        lambda: im.find_sources(image),                                          # no noise
        lambda: im.find_sources(image.to(torch.float32), noise=1.0),
        lambda: im.find_sources(image, beam=np.zeros(8), noise=1.0),
        lambda: im.find_sources(image, noise=1.0, out=np.zeros((1024, 10))),
        lambda: ctx.find_sources(theta, lam, image, beam=np.zeros(8), noise=1.0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"


# ---- the restatement on cases computed by hand ---------------------------------------------------------------------------
FIXED = dict(sigma=None, nsigma=(0.0, 0.0))


def test_a_single_cell():
    """N = 5 (N/2 = 2), theta 0.1: one cell of 3 at (y, x) = (1, 3).  Every moment about the peak is 0: a point at l =
    0.1 (3 - 2) / 5, m = 0.1 (1 - 2) / 5 with F = 3; cut at T_lo = 0.75, t = 1/4 and the corrected flux is 3 / 0.75 = 4."""
    img = np.zeros((5, 5))
    img[1, 3] = 3.0
    r = sources_ref.find_sources(img, 0.1, thr=(1.0, 0.75), correct=False, **FIXED)
    assert r["count"] == 1
    assert np.array_equal(r["info"][0], [8, 1, 1, 3, 3.0, 3.0, 0, 0, 0, 0, 0, 1, 1, 3, 3, 1])
    assert np.array_equal(r["comps"][0], [0.1 * 1.0 / 5, 0.1 * -1.0 / 5, 3.0, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(r["stats"], [1.0, 0.75, 3.0, 1, 1, 1, 3.0, 0])
    r = sources_ref.find_sources(img, 0.1, thr=(1.0, 0.75), correct=True, **FIXED)
    assert r["comps"][0, 2] == 4.0 and r["info"][0, 15] == 1
    # a level of 0: t = 0 and the correction leaves everything as it is
    r = sources_ref.find_sources(img, 0.1, thr=(0.0, 0.0), correct=True, **FIXED)
    assert r["comps"][0, 2] == 3.0
    # on the rim, or inside a border that the box touches: the edge bit
    img = np.zeros((5, 5))
    img[0, 2] = img[2, 2] = 1.0
    r = sources_ref.find_sources(img, 0.1, thr=(0.5, 0.5), correct=False, **FIXED)
    assert r["info"][:, 15].tolist() == [3, 1]
    r = sources_ref.find_sources(img, 0.1, border=1, thr=(0.5, 0.5), correct=False, **FIXED)
    assert r["count"] == 1 and r["info"][0, 0] == 12 and r["info"][0, 15] == 1
    r = sources_ref.find_sources(img, 0.1, border=2, thr=(0.5, 0.5), correct=False, **FIXED)
    assert r["count"] == 1 and r["info"][0, 15] == 3


def test_a_two_by_three_block():
    """N = 8 (N/2 = 4), theta 0.1: ones on rows 2-3, columns 1-3.  The peak is the first cell (2, 1); dx = 0, 1, 2 and dy =
    0, 1: S = 6, Sx = 6, Sy = 3, Sxx = 2 (0 + 1 + 4) = 10, Sxy = 0 + 1 + 2 = 3, Syy = 3.  cx = 1 + 1 = 2, cy = 2.5; mxx =
    10/6 - 1 = 2/3, mxy = 3/6 - 1 * 0.5 = 0, myy = 3/6 - 0.25 = 0.25: the major axis along x (from +m towards +l: bpa = pi/2),
    FWHM = sqrt(8 ln 2 lambda) cells."""
    img = np.zeros((8, 8))
    img[2:4, 1:4] = 1.0
    r = sources_ref.find_sources(img, 0.1, thr=(0.5, 0.5), correct=False, **FIXED)
    assert r["count"] == 1
    assert np.array_equal(r["info"][0], [17, 6, 2, 1, 1.0, 6, 6, 3, 10, 3, 3, 2, 3, 1, 3, 0])
    l, m, F, _, _, _, bmaj, bmin, bpa, _ = r["comps"][0]
    assert l == 0.1 * (2.0 - 4.0) / 8 and m == 0.1 * (2.5 - 4.0) / 8 and F == 6.0
    c = 8.0 * math.log(2.0)
    assert bmaj == pytest.approx(math.sqrt(c * 2.0 / 3.0) * 0.1 / 8, rel=1e-14)
    assert bmin == pytest.approx(math.sqrt(c * 0.25) * 0.1 / 8, rel=1e-14)
    assert bpa == 0.5 * math.pi
    assert sources_ref.shape_covariance(bmaj, bmin, bpa, 0.1, 8) == pytest.approx((2.0 / 3.0, 0.0, 0.25), abs=1e-15)
    # turned: 3 x 2, the major axis along y: bpa = 0
    r = sources_ref.find_sources(img.T, 0.1, thr=(0.5, 0.5), correct=False, **FIXED)
    assert r["comps"][0, 8] == 0.0 and r["comps"][0, 6] == pytest.approx(bmaj, rel=1e-14)
    # a beam with the block's own covariance in x and more in y: iyy < 0, a point; the flux is S sqrt(det) / pi
    A, Cc = 1.0 / (2.0 * 0.5), 1.0 / (2.0 * 0.5)
    beam = [A, 0.0, Cc, 0, 0, 0, 8, 1.0]
    assert sources_ref.beam_covariance(beam) == (0.5, 0.0, 0.5)
    r = sources_ref.find_sources(img, 0.1, thr=(0.5, 0.5), beam=beam, correct=False, **FIXED)
    assert r["info"][0, 15] == 1 and np.array_equal(r["comps"][0, 6:9], [0, 0, 0])
    assert r["comps"][0, 2] == 6.0 * math.sqrt(1.0) / math.pi
    assert r["cov"][0].tolist() == pytest.approx([2.0 / 3.0 - 0.5, 0.0, -0.25], abs=1e-15)
    # a narrower beam is deconvolved: ixx = 2/3 - 1/8, iyy = 1/4 - 1/8
    beam = [4.0, 0.0, 4.0, 0, 0, 0, 8, 1.0]
    r = sources_ref.find_sources(img, 0.1, thr=(0.5, 0.5), beam=beam, correct=False, **FIXED)
    assert r["info"][0, 15] == 0 and r["cov"][0].tolist() == pytest.approx([2.0 / 3.0 - 0.125, 0.0, 0.125], abs=1e-15)
    assert r["comps"][0, 2] == 6.0 * 4.0 / math.pi
    # an unusable beam: NaN in flux and shape, the position stands, flag bit 2 and not the point bit
    for bad in ([4.0, 0.0, 4.0, 0, 0, 0, 8, 0.0], [1.0, 2.0, 1.0, 0, 0, 0, 8, 1.0], [nan, 0.0, 4.0, 0, 0, 0, 8, 1.0]):
        r = sources_ref.find_sources(img, 0.1, thr=(0.5, 0.5), beam=bad, correct=False, **FIXED)
        assert r["info"][0, 15] == 4 and np.all(np.isnan(r["comps"][0, [2, 6, 7, 8]])) and r["comps"][0, 0] == l
        assert np.isnan(r["stats"][6]) and r["stats"][5] == 0


def test_two_islands_in_label_order_and_a_dropped_one():
    """7 x 7.  Island A: (1, 4) = 2 and (1, 5) = 4; island B: (3, 0) = 3, (4, 1) = 5 (touching diagonally).  B's first cell
    has the larger index: A is row 0.  A third island at (6, 6) = 2.5 with thr_hi = 2.75 holds no cell above T_hi at all; and
    with min_cells = 2 at thr = (2.5, 1) A's only H cell, (1, 5), is a pruned component: A is dropped, B (whose two cells
    are both above 2.5) stays."""
    img = np.zeros((7, 7))
    img[1, 4], img[1, 5] = 2.0, 4.0
    img[3, 0], img[4, 1] = 3.0, 5.0
    r = sources_ref.find_sources(img, 0.1, thr=(1.0, 1.0), correct=False, **FIXED)
    assert r["count"] == 2
    # A: the peak is (1, 5); the other cell lies at dx = -1: Sx = -2, Sxx = 2
    assert np.array_equal(r["info"][0], [11, 2, 1, 5, 4.0, 6, -2, 0, 2, 0, 0, 1, 1, 4, 5, 1])
    # B: the peak is (4, 1); the other cell at dx = -1, dy = -1: Sx = Sy = -3, Sxx = Sxy = Syy = 3; the box touches x = 0
    assert np.array_equal(r["info"][1], [21, 2, 4, 1, 5.0, 8, -3, -3, 3, 3, 3, 3, 4, 0, 1, 3])
    assert np.array_equal(r["stats"], [1.0, 1.0, 5.0, 2, 2, 2, 14.0, 0])
    # max_c = 1: the count is still 2, one row
    r = sources_ref.find_sources(img, 0.1, thr=(1.0, 1.0), correct=False, max_c=1, **FIXED)
    assert r["count"] == 2 and r["comps"].shape == (1, 10) and np.array_equal(r["stats"][3:7], [2, 1, 1, 6.0])
    img[6, 6] = 2.5
    r = sources_ref.find_sources(img, 0.1, thr=(2.75, 1.0), correct=False, **FIXED)
    assert r["info"][:, 0].tolist() == [11, 21]
    r = sources_ref.find_sources(img, 0.1, thr=(2.5, 1.0), min_cells=2, correct=False, **FIXED)
    assert r["info"][:, 0].tolist() == [21]
    # two equal peaks: the smaller index is the peak
    img[3, 0] = 5.0
    r = sources_ref.find_sources(img, 0.1, thr=(4.5, 4.5), correct=False, **FIXED)
    assert r["info"][0, :5].tolist() == [21, 2, 3, 0, 5.0]
    # reasons: a NaN sigma is 3, nothing taking part 2; no rows, count 0
    r = sources_ref.find_sources(img, 0.1, sigma=np.nan)
    assert r["count"] == 0 and r["stats"][7] == 3 and np.isnan(r["stats"][0]) and r["stats"][2] == 5.0
    r = sources_ref.find_sources(np.full((7, 7), np.nan), 0.1, thr=(1.0, 1.0), **FIXED)
    assert r["count"] == 0 and r["stats"][7] == 2 and r["comps"].shape == (0, 10)


def test_the_angle_series():
    """atan2 from +, -, *, / alone (the header states the steps): exact where the answer is a multiple of pi / 4, and within
    1e-15 relative of math.atan2 - the roundings it is made of: the quotient t, the reduction (three), the 23-term Horner
    sum (whose terms fall by z <= 0.172 each, so about one), t s, the base and the two reflections, half a unit each."""
    pi = math.pi
    for y, x, want in ((0.0, 1.0, 0.0), (0.0, -1.0, pi), (1.0, 0.0, 0.5 * pi), (-1.0, 0.0, -0.5 * pi), (1.0, 1.0, 0.25 * pi),
                       (0.0, 0.0, 0.0), (-3.0, -3.0, -(pi - 0.25 * pi))):
        assert sources_ref.atan2_series(y, x) == want, (y, x)
    rng = np.random.default_rng(3)
    ys = rng.uniform(-1, 1, 20000) * 10.0 ** rng.uniform(-6, 6, 20000)
    xs = rng.uniform(-1, 1, 20000) * 10.0 ** rng.uniform(-6, 6, 20000)
    worst = max(abs(sources_ref.atan2_series(y, x) - math.atan2(y, x)) / abs(math.atan2(y, x)) for y, x in zip(ys, xs))
    print(worst)
    assert worst <= 1e-15


# ---- the restatement against truth ---------------------------------------------------------------------------------------
def gaussian_covariance(fmaj, fmin, angle):
    """the covariance matrix [[xx, xy], [xy, yy]] in cells^2 of FWHMs fmaj, fmin with the major axis at `angle` from +x"""
    c = 8.0 * math.log(2.0)
    lp, lm, cs, sn = fmaj ** 2 / c, fmin ** 2 / c, math.cos(angle), math.sin(angle)
    return np.array([[lp * cs * cs + lm * sn * sn, (lp - lm) * cs * sn], [(lp - lm) * cs * sn, lp * sn * sn + lm * cs * cs]])


def beam_of(cov):
    """the 8 doubles of a beam with this covariance: [[A, B], [B, C]] = inverse(cov) / 2"""
    q = np.linalg.inv(cov) / 2.0
    return [q[0, 0], q[0, 1], q[1, 1], 0.0, 0.0, 0.0, 0.0, 1.0]


def convolved_gaussian(N, flux, intrinsic, beamcov, centre):
    """An elliptical Gaussian of integrated flux `flux` (per cell area) and covariance `intrinsic`, convolved analytically
    with the unit-peak beam of covariance `beamcov` and sampled on the grid: a Gaussian of covariance intrinsic + beamcov
    and peak flux sqrt(det beamcov / det (intrinsic + beamcov)), in units per beam."""
    total = intrinsic + beamcov
    inv = np.linalg.inv(total)
    yy, xx = np.mgrid[0:N, 0:N]
    dx, dy = xx - centre[0], yy - centre[1]
    peak = flux * math.sqrt(np.linalg.det(beamcov) / np.linalg.det(total))
    return peak * np.exp(-0.5 * (inv[0, 0] * dx * dx + 2.0 * inv[0, 1] * dx * dy + inv[1, 1] * dy * dy)), peak


def test_the_restatement_recovers_analytic_gaussians():
    """Isolated, noise-free Gaussians - intrinsic FWHM 3, 5, 8 cells, axis ratio 1, 2, 3, four angles - convolved with a beam
    of 3.5 x 2.5 cells at 20 degrees, centred off the grid at (+0.3, -0.2) cells, cut at t = 0.05, 0.15, 0.3 of the true peak.
    correct = 1 recovers flux, position and intrinsic covariance up to what sampling does to a cut: the cells above the level
    are a staircase, not an ellipse, and t is taken from the peak CELL.  The bounds are twice the worst deviations of this
    restatement over these 108 cases, measured on the CPU when the test was written: flux 6.11e-2 relative (at FWHM 3, ratio
    1, t = 0.3: 27 cells), position 0.120 cells, covariance 9.90e-2 of the trace of the observed covariance.  correct = 0
    leaves the flux low by the factor 1 - t: measured within 3.59e-2 of it."""
    N, theta, flux, off = 64, 0.1, 2.0, (0.3, -0.2)
    beamcov = gaussian_covariance(3.5, 2.5, math.radians(20.0))
    beam = beam_of(beamcov)
    assert sources_ref.beam_covariance(beam) == pytest.approx((beamcov[0, 0], beamcov[0, 1], beamcov[1, 1]), rel=1e-12)
    centre = (N // 2 + off[0], N // 2 + off[1])
    worst = dict(flux=0.0, position=0.0, covariance=0.0, uncorrected=0.0)
    for fmaj, ratio, angle, t in itertools.product((3.0, 5.0, 8.0), (1.0, 2.0, 3.0), (0.0, 30.0, 75.0, 120.0), (0.05, 0.15, 0.3)):
        intrinsic = gaussian_covariance(fmaj, fmaj / ratio, math.radians(angle))
        img, peak = convolved_gaussian(N, flux, intrinsic, beamcov, centre)
        T = t * peak
        r = sources_ref.find_sources(img, theta, thr=(T, T), beam=beam, correct=True, **FIXED)
        assert r["count"] == 1 and r["info"][0, 15] == 0, (fmaj, ratio, angle, t)
        l, m, F = r["comps"][0, :3]
        px, py = l * N / theta + N // 2 - centre[0], m * N / theta + N // 2 - centre[1]
        cov = r["cov"][0]
        dev = max(abs(cov[0] - intrinsic[0, 0]), abs(cov[1] - intrinsic[0, 1]), abs(cov[2] - intrinsic[1, 1]))
        worst["flux"] = max(worst["flux"], abs(F - flux) / flux)
        worst["position"] = max(worst["position"], math.hypot(px, py))
        worst["covariance"] = max(worst["covariance"], dev / np.trace(intrinsic + beamcov))
        # the shape fields say the same covariance
        back = sources_ref.shape_covariance(*r["comps"][0, 6:9], theta, N)
        assert back == pytest.approx(tuple(cov), rel=1e-10, abs=1e-12)
        r0 = sources_ref.find_sources(img, theta, thr=(T, T), beam=beam, correct=False, **FIXED)
        worst["uncorrected"] = max(worst["uncorrected"], abs(r0["comps"][0, 2] / flux - (1.0 - t)))
    print(worst)
    assert worst["flux"] <= 2 * 6.11e-2 and worst["position"] <= 2 * 0.120 and worst["covariance"] <= 2 * 9.90e-2
    assert worst["uncorrected"] <= 2 * 3.59e-2
    # Finely sampled the same estimator converges: FWHM 24 x 12 cells, t = 0.15.  The staircase is a band of about one cell
    # along the cut, so its share of the island falls as perimeter / area, as 1 / sqrt(ncells): the bounds above, which
    # held at 16 cells and more, scaled by sqrt(16 / ncells).
    N = 160
    intrinsic = gaussian_covariance(24.0, 12.0, math.radians(30.0))
    beamcov = gaussian_covariance(10.0, 8.0, math.radians(20.0))
    img, peak = convolved_gaussian(N, flux, intrinsic, beamcov, (N // 2 + 0.3, N // 2 - 0.2))
    r = sources_ref.find_sources(img, theta, thr=(0.15 * peak,) * 2, beam=beam_of(beamcov), correct=True, **FIXED)
    cov, scale = r["cov"][0], math.sqrt(16.0 / r["info"][0, 1])
    dev = max(abs(cov[0] - intrinsic[0, 0]), abs(cov[1] - intrinsic[0, 1]), abs(cov[2] - intrinsic[1, 1]))
    print(r["info"][0, 1], abs(r["comps"][0, 2] - flux) / flux, dev / np.trace(intrinsic + beamcov))
    assert r["info"][0, 1] > 500  # (against 16 to 63 cells above)
    assert abs(r["comps"][0, 2] - flux) / flux <= 2 * 6.11e-2 * scale
    assert dev / np.trace(intrinsic + beamcov) <= 2 * 9.90e-2 * scale
