"""Auto-masking (gridhip_automask*, gridhip_imager_[ms]deconvolve_automask_dev), the checks that need no GPU: the library,
the header, the ctypes table and the bindings carry every new name; NULL handles and every argument the header refuses
are refused with nothing touched; the Python methods hand the ABI the right pointers and order (against a recording
library) and still take today's entry points when `automask` is left alone; and the restatement the GPU tests compare
with (tests/automask_ref.py) is right on cases computed by hand and agrees with scipy's labelling where scipy is there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import automask_cases
import automask_ref
from conftest import ROOT
from test_binding_marshalling import HANDLE, Arr, Out, Same
from test_clean_host import SameT, rig, tensor_returned, torch_rig  # noqa: F401  (fixtures)
from test_noise_host import ScalesArr

NAMES = ["gridhip_automask", "gridhip_automask_dev", "gridhip_imager_automask_dev",
         "gridhip_imager_deconvolve_automask_dev", "gridhip_imager_msdeconvolve_automask_dev"]
f64 = np.float64


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
    assert _lib.SIGNATURES["gridhip_automask"] == _lib.SIGNATURES["gridhip_automask_dev"]
    assert "auto-masking" in text and _lib.load().gridhip_version() >= 230
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", text).group(1)) >= 230


def test_bindings_carry_the_names():
    import gridhip
    for cls in (gridhip.Context, gridhip.Imager):
        assert callable(cls.automask)
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("automaskIO", "imagerDeconvolveAutomaskIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper
    hpp = open(os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host", "gridding.hpp")).read()
    assert "gridhip_automask(" in hpp


class Call:
    """one call of the three automask forms on host arrays that must come back untouched"""

    def __init__(self, N=8):
        self.N = N
        self.image, self.mask = np.full(N * N, 1.5), np.full(N * N, 5, dtype=np.uint8)
        self.stats, self.noise = np.full(8, 7.0), np.full(1, 9.0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self.kw = dict(N=N, image=p(self.image), mask=p(self.mask), border=0, absolute=0, thr_hi=1.0, thr_lo=0.5,
                       nsigma_hi=5.0, nsigma_lo=2.5, noise=p(self.noise), peak_frac=0.1, min_cells=1, grow=1,
                       stats=p(self.stats))

    def args(self, **change):
        kw = dict(self.kw, **change)
        return [kw[k] for k in ("N", "image", "mask", "border", "absolute", "thr_hi", "thr_lo", "nsigma_hi", "nsigma_lo",
                                "noise", "peak_frac", "min_cells", "grow", "stats")]

    def untouched(self):
        return (np.all(self.image == 1.5) and np.all(self.mask == 5) and np.all(self.stats == 7.0)
                and self.noise[0] == 9.0)


def test_null_handles_are_refused_and_nothing_is_touched():
    from gridhip import _lib
    lib = _lib.load()
    c = Call()
    a = c.args()
    assert lib.gridhip_automask(None, *a) == _lib.EINVAL
    assert lib.gridhip_automask_dev(None, *a) == _lib.EINVAL
    assert lib.gridhip_imager_automask_dev(None, *a[1:]) == _lib.EINVAL
    cl = (0.1, 0.0, 5, 0, 0)
    loop = (a[2], 3.0, 0.1, 0, 1.0, 0.5, 5.0, 2.5, 0.1, 1, 1, a[-1], a[-1], a[-1])
    sc = (C.c_double * 2)(0.0, 2.0)
    assert lib.gridhip_imager_deconvolve_automask_dev(None, a[1], a[1], a[1], 2, *cl, *loop) == _lib.EINVAL
    assert lib.gridhip_imager_msdeconvolve_automask_dev(None, a[1], a[1], a[1], 2, 2, sc, sc, *cl, *loop) == _lib.EINVAL
    assert c.untouched()


nan, inf = float("nan"), float("inf")
EINVAL_CASES = [
    dict(thr_hi=0.25), dict(nsigma_lo=6.0),                                      # lo above hi
    dict(thr_hi=-1.0, thr_lo=-2.0), dict(thr_lo=-0.5), dict(thr_hi=inf), dict(thr_hi=nan), dict(thr_lo=nan),
    dict(nsigma_hi=inf), dict(nsigma_hi=nan), dict(nsigma_lo=-1.0), dict(nsigma_lo=nan),
    dict(peak_frac=1.0), dict(peak_frac=-0.1), dict(peak_frac=nan),
    dict(noise=None),                                                            # nsigma_hi > 0 with NULL noise
    dict(min_cells=0), dict(min_cells=-3), dict(grow=-1),
    dict(image=None), dict(mask=None), dict(stats=None),
    dict(N=0), dict(N=-1), dict(border=4), dict(border=5), dict(border=-1),     # 2 * border >= N = 8
]


def test_every_refused_argument_with_a_null_handle_touches_nothing():
    """A context cannot be made without a GPU, so what a host can see of the argument rules is this: whatever else is
    wrong with a call, a NULL handle is refused first and nothing is read or written.  The rules themselves are checked
    with a context in tests/test_gpu_automask.py::test_refusals, over the same list."""
    from gridhip import _lib
    lib = _lib.load()
    c = Call()
    for change in EINVAL_CASES + [dict(grow=33), dict(N=46341)]:
        a = c.args(**change)
        assert lib.gridhip_automask(None, *a) == _lib.EINVAL, change
        assert lib.gridhip_automask_dev(None, *a) == _lib.EINVAL, change
        assert lib.gridhip_imager_automask_dev(None, *a[1:]) == _lib.EINVAL, change
    assert c.untouched()


# ---- the restatement on cases computed by hand ---------------------------------------------------------------------------
def test_labelling_on_hand_computed_cases():
    s = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 0],
                  [0, 0, 0, 1],
                  [1, 0, 1, 0]], dtype=bool)
    # (0,0)-(1,1) touch diagonally: label 0.  (0,3) alone: 3.  (2,3)-(3,2) diagonally: 11.  (3,0) alone: 12.
    want = np.array([[0, -1, -1, 3], [-1, 0, -1, -1], [-1, -1, -1, 11], [12, -1, 11, -1]])
    assert np.array_equal(automask_ref.label(s), want)
    board = np.indices((5, 5)).sum(0) % 2 == 0
    assert np.array_equal(np.unique(automask_ref.label(board)), [-1, 0])  # one component under 8-connectivity
    u = np.zeros((4, 4), dtype=bool)
    u[:, 0] = u[:, 3] = u[3, :] = True
    assert np.array_equal(np.unique(automask_ref.label(u)), [-1, 0])
    assert np.array_equal(automask_ref.label(np.zeros((2, 2), dtype=bool)), np.full((2, 2), -1))


def test_automask_on_a_hand_computed_case():
    """6 x 6.  An island of three cells at 4 (row 1, columns 1-3) inside a longer one at 2 (row 1, columns 0-4); a lone
    cell at 4 at (4, 4) with a neighbour at 2 at (4, 5).  thr = (3, 1), min_cells = 2: H has two components (3 cells and
    1), one survives; L has two, and only the one around the surviving seeds is kept: 5 cells.  grow 1 makes that rows
    0-2, columns 0-5: 18 cells.  The mask starts with a 7 at (0, 0), which stays 7: 17 cells newly set."""
    img = np.zeros((6, 6))
    img[1, 0:5] = 2.0
    img[1, 1:4] = 4.0
    img[4, 4], img[4, 5] = 4.0, 2.0
    mask = np.zeros((6, 6), dtype=np.uint8)
    mask[0, 0] = 7
    out, st = automask_ref.automask(img, mask, None, thr=(3.0, 1.0), nsigma=(0.0, 0.0), min_cells=2, grow=1)
    want = np.zeros((6, 6), dtype=np.uint8)
    want[0:3, :] = 1
    want[0, 0] = 7
    assert np.array_equal(out, want) and mask[0, 0] == 7 and mask.sum() == 7
    assert np.array_equal(st, [3.0, 1.0, 4.0, 2.0, 1.0, 1.0, 17.0, 0.0])
    # min_cells 1: both islands; no grow: 5 + 2 cells, the 7 is outside both
    out, st = automask_ref.automask(img, mask, None, thr=(3.0, 1.0), nsigma=(0.0, 0.0))
    assert out.sum() == 7 + 7 and np.array_equal(st[3:], [2.0, 2.0, 2.0, 7.0, 0.0])
    # the levels: sigma 0.5, nsigma (7, 3) -> 3.5 and 1.5; peak_frac 0.9 lifts both to 3.6, each product rounded once
    out, st = automask_ref.automask(img, mask, 0.5, nsigma=(7.0, 3.0))
    assert np.array_equal(st[:3], [3.5, 1.5, 4.0]) and st[6] == 7
    out, st = automask_ref.automask(img, mask, 0.5, nsigma=(7.0, 3.0), peak_frac=0.9)
    assert np.array_equal(st[:2], [0.9 * 4.0, 0.9 * 4.0]) and st[6] == 4  # H = L = the four cells at 4
    # a border of 1 takes (4, 5) and (1, 0) out; a NaN sigma is reason 3, an all-NaN image reason 2: the mask untouched
    out, st = automask_ref.automask(img, mask, None, border=1, thr=(3.0, 1.0), nsigma=(0.0, 0.0), grow=1)
    assert not out[0, 1:].any() and not out[:, 5].any() and out[1, 1] == 1 and out[0, 0] == 7
    out, st = automask_ref.automask(img, mask, np.nan)
    assert np.array_equal(out, mask) and st[7] == 3 and np.isnan(st[0]) and np.isnan(st[1]) and st[2] == 4.0
    out, st = automask_ref.automask(np.full((6, 6), np.nan), mask, None, thr=(3.0, 1.0), nsigma=(0.0, 0.0))
    assert np.array_equal(out, mask) and st[7] == 2 and np.isnan(st[2]) and np.array_equal(st[:2], [3.0, 1.0])
    # absolute: a negative island counts; strictness: a cell AT the level is not above it
    neg = -img
    out, st = automask_ref.automask(neg, mask, None, thr=(3.0, 1.0), nsigma=(0.0, 0.0))
    assert st[3] == 0 and out.sum() == 7
    out, st = automask_ref.automask(neg, mask, None, absolute=True, thr=(3.0, 1.0), nsigma=(0.0, 0.0))
    assert st[3] == 2 and st[2] == 4.0
    out, st = automask_ref.automask(img, mask, None, thr=(4.0, 2.0), nsigma=(0.0, 0.0))
    assert st[3] == 0 and st[6] == 0


@pytest.mark.parametrize("N", automask_cases.sizes())
def test_the_labelling_agrees_with_scipy(N):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, inset in automask_cases.patterns(N).items():
        lab, n = ndimage.label(inset, structure=np.ones((3, 3)))
        mine = automask_ref.label(inset)
        assert np.array_equal(mine >= 0, inset), name
        assert np.unique(mine[mine >= 0]).size == n, name
        for c in range(1, n + 1):  # each of scipy's components carries one label here: its smallest flat index
            cells = np.flatnonzero(lab == c)
            assert np.all(mine.flat[cells] == cells.min()), (name, c)


def test_the_cases_hold_what_they_are_for():
    th, tw = automask_cases.tile()
    assert automask_cases.sizes() == [1, 2, 3, tw - 1, tw + 1, 2 * tw + 3]
    N = 2 * tw + 3
    p = automask_cases.patterns(N)
    for name in ("checkerboard", "diagonal across four tiles", "anti-diagonal across four tiles", "U", "serpentine",
                 "serpentine, upright"):
        lab = automask_ref.label(p[name])
        assert np.unique(lab[lab >= 0]).size == 1, name
    s = p["serpentine"]  # crosses every tile, several times
    for ty in range(0, N, th):
        for tx in range(0, N, tw):
            rows = s[ty:ty + th, tx:tx + tw].all(axis=1)
            assert rows.sum() >= 1 and (rows.sum() >= 3 or ty + th > N), (ty, tx)
    lab = automask_ref.label(p["cut by each tile edge"])
    assert np.unique(lab[lab >= 0]).size == 4
    names = [c[0] for c in automask_cases.feature_cases()]
    assert len(set(names)) == len(names)


# ---- what the Python methods hand to the ABI ------------------------------------------------------------------------------
def test_context_automask_host_form(rig):
    ctx, rec, run = rig
    N = 6
    image = np.arange(N * N, dtype=f64).reshape(N, N)
    mask8 = np.zeros((N, N), dtype=np.uint8)
    maskb = np.zeros((N, N), dtype=bool)
    st = Out(f64, 8)
    m, s = run(lambda: ctx.automask(image, mask8, 0.125, border=1, absolute=True, thr=(2, 1), nsigma=(6, 3), peak_frac=0.25,
                                    min_cells=4, grow=2),
               "gridhip_automask", N, Same(image), Same(mask8), 1, 1, 2.0, 1.0, 6.0, 3.0, Arr([0.125], f64), 0.25, 4, 2, st)
    assert m is mask8 and st.returned(s, (8,))
    # defaults; a bool mask goes as its own bytes and comes back as it is; one element of a stats array by its own address
    stats = np.arange(8, dtype=f64)
    st = Out(f64, 8)
    m, s = run(lambda: ctx.automask(image, maskb, stats[3:4]), "gridhip_automask", N, Same(image), Same(maskb), 0, 0,
               0.0, 0.0, 5.0, 2.5, Same(stats, 24), 0.0, 1, 0, st)
    assert m is maskb and st.returned(s, (8,))
    # no mask: a new one of zeros, uint8, returned; fixed levels need no noise; a float32 image is converted
    z, st = Out(np.uint8, N * N), Out(f64, 8)
    m, s = run(lambda: ctx.automask(image.astype(np.float32), thr=1.5, nsigma=0), "gridhip_automask", N, Arr(image, f64),
               z, 0, 0, 1.5, 1.5, 0.0, 0.0, None, 0.0, 1, 0, st)
    assert z.returned(m, (N, N)) and st.returned(s, (8,))
    bad = [
        lambda: ctx.automask(image, mask8),                                # nsigma > 0 and no noise
        lambda: ctx.automask(image, mask8, 1.0, nsigma=(2, 3)),            # lo above hi
        lambda: ctx.automask(image, mask8, 1.0, thr=(-1, -1)),
        lambda: ctx.automask(image, mask8, 1.0, thr=(float("inf"), 0)),
        lambda: ctx.automask(image, mask8, 1.0, peak_frac=1.0),
        lambda: ctx.automask(image, mask8, 1.0, min_cells=0),
        lambda: ctx.automask(image, mask8, 1.0, grow=-1),
        lambda: ctx.automask(image, mask8, 1.0, grow=33),
        lambda: ctx.automask(image, mask8.astype(np.int32), 1.0),
        lambda: ctx.automask(image, mask8[:, :5], 1.0),
        lambda: ctx.automask(image, np.zeros((N, 2 * N), dtype=np.uint8)[:, ::2], 1.0),   # not contiguous: no copy
        lambda: ctx.automask(image, mask8, np.zeros(2)),
        lambda: ctx.automask(np.zeros((N, N + 1)), None, 1.0),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert rec.calls.count("gridhip_automask") == 3


def test_imager_forms(torch_rig):
    import torch
    ctx, im, rec, run, bound, be = torch_rig
    N, n, h = im.N, im.n, im._h
    image = torch.arange(N * N, dtype=torch.float64).reshape(N, N)
    model = torch.ones((N, N), dtype=torch.float64)
    vis = torch.arange(n, dtype=torch.float64).to(torch.complex128)
    mask = torch.zeros((N, N), dtype=torch.bool)
    mask8 = torch.zeros((N, N), dtype=torch.uint8)
    sig = torch.arange(8, dtype=torch.float64)
    st = Out(f64, 8)
    m, s = run(lambda: im.automask(image, mask, sig[3:4], 1, True, (2, 1), (6, 3), 0.25, 4, 2), "gridhip_imager_automask_dev",
               SameT(image), SameT(mask), 1, 1, 2.0, 1.0, 6.0, 3.0, SameT(sig[3:4]), 0.25, 4, 2, st, handle=h)
    assert m is mask and tensor_returned(st, s, (8,)) and bound == [ctx]
    st = Out(f64, 8)
    m, s = run(lambda: ctx.automask(image, mask8, nsigma=0, thr=(3, 1)), "gridhip_automask_dev", N, SameT(image),
               SameT(mask8), 0, 0, 3.0, 1.0, 0.0, 0.0, None, 0.0, 1, 0, st)
    assert m is mask8 and tensor_returned(st, s, (8,))
    # the loop: the three tables, one row per major cycle, and the mask handed back
    st, ist, ast = Out(f64, 3 * 8), Out(f64, 3 * 8), Out(f64, 3 * 8)
    out = run(lambda: im.deconvolve(vis, 3, model=model, gain=0.25, threshold=0.5, niter=7, border=1, patch=2, mask=mask8,
                                    nsigma=3.0, peak_frac=0.1,
                                    automask=dict(absolute=True, thr=(2, 1), nsigma=(6, 3), peak_frac=0.25, min_cells=4,
                                                  grow=2)),
              "gridhip_imager_deconvolve_automask_dev", SameT(vis), SameT(model), Out(f64, N * N), 3, 0.25, 0.5, 7, 1, 2,
              SameT(mask8), 3.0, 0.1, 1, 2.0, 1.0, 6.0, 3.0, 0.25, 4, 2, st, ist, ast, handle=h)
    assert len(out) == 6 and out[0] is model and out[4] is mask8
    assert tensor_returned(st, out[2], (3, 8)) and tensor_returned(ist, out[3], (3, 8)) and tensor_returned(ast, out[5], (3, 8))
    # defaults, msclean as the minor cycle, a mask of the method's own
    z = Out(np.uint8, N * N)
    out = run(lambda: im.deconvolve(vis, 2, model=model, scales=[0.0, 2.0], automask={}),
              "gridhip_imager_msdeconvolve_automask_dev", SameT(vis), SameT(model), Out(f64, N * N), 2, 2,
              ScalesArr([0.0, 2.0]), ScalesArr([1.0, 0.4]), 0.1, 0.0, 100, 0, 0, z, 0.0, 0.0, 0, 0.0, 0.0, 5.0, 2.5, 0.0, 1,
              0, Out(f64, 2 * 16), Out(f64, 2 * 8), Out(f64, 2 * 8), handle=h)
    assert tuple(out[2].shape) == (2, 16) and tuple(out[3].shape) == (2, 8) and tuple(out[5].shape) == (2, 8)
    assert out[4].dtype == torch.uint8 and np.array_equal(out[4].numpy().ravel(), z.fill)
    # `automask` left alone: today's entry points with today's arguments
    run(lambda: im.deconvolve(vis, 2, model=model), "gridhip_imager_deconvolve_dev", SameT(vis), SameT(model),
        Out(f64, N * N), 2, 0.1, 0.0, 100, 0, 0, Out(f64, 8), handle=h)
    out = run(lambda: im.deconvolve(vis, 2, model=model, mask=mask, nsigma=3.0), "gridhip_imager_deconvolve_auto_dev",
              SameT(vis), SameT(model), Out(f64, N * N), 2, 0.1, 0.0, 100, 0, 0, SameT(mask), 3.0, 0.0, Out(f64, 16),
              Out(f64, 16), handle=h)
    assert len(out) == 4
    run(lambda: im.deconvolve(vis, 2, model=model, scales=[0.0, 2.0]), "gridhip_imager_msdeconvolve_dev", SameT(vis),
        SameT(model), Out(f64, N * N), 2, 2, ScalesArr([0.0, 2.0]), ScalesArr([1.0, 0.4]), 0.1, 0.0, 100, 0, 0,
        Out(f64, 24), handle=h)
    before = len(rec.calls)
    bad = [
        lambda: im.automask(image, mask8),                                   # no noise
        lambda: im.automask(image, mask8.to(torch.int32), 1.0),
        lambda: im.automask(image, np.zeros((N, N), dtype=np.uint8), 1.0),
        lambda: im.automask(image.to(torch.float32), mask8, 1.0),
        lambda: im.deconvolve(vis, 2, automask=dict(grows=1)),
        lambda: im.deconvolve(vis, 2, automask=dict(nsigma=(1, 2))),
        lambda: im.deconvolve(vis, 2, automask={}, peak_frac=1.5),
        lambda: im.deconvolve(vis, 2, automask={}, mask=mask8[:5, :5].contiguous()),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(rec.calls) == before, f"refusal {k} came after {rec.calls[before:]}"
