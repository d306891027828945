"""The three minor-cycle loops on the device - gridhip_clean*, gridhip_msclean* and gridhip_mfclean* - at the inputs the
seeded skies of the other clean tests never reach: exact ties at every level of the reductions, more tiles than the pick
kernel has threads, components on the image's rim, N from 1 up, bases 8 bytes off a 16-byte boundary, special values.
The fixtures and their preconditions are tests/clean_edge_cases.py and tests/test_clean_edges_host.py.

Tolerance: none for the exact fixtures - model, residual and stats are the restatement's bits (the host test shows that
no operation of those runs rounds, so nothing a kernel fuses can change them) - through Hogbom, through msclean with
scales = [0] and through mfclean with T = 1, which each carry their own copy of the tile code - and through msclean
with scales = [0, 1] and equal biases, where every pick is an exact tie between the two scales.

The wide forms (msclean with scales = [0, 2] and [0, 32], mfclean with T = 2 and 3) round: identical iteration counts,
per-scale counts, component positions and final index, values within the project's 1e-10 of the peak (the compare
functions of test_gpu_msclean.py and test_gpu_mfclean.py).  Their ties are made by translation - identical stamps - which
keeps every bit equal at the stamps on each side separately; the host test asserts on the restatement's trace that the
gap is exactly 0 at the tied picks and above 1e-8 at every other."""
import functools

import numpy as np
import pytest

import clean_edge_cases as E
from test_gpu_imager import host, to_dev
from test_gpu_mfclean import compare as compare_mf
from test_gpu_msclean import compare as compare_ms

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0

TIES = E.tie_fixtures()
RIM = E.rim_fixtures() + E.straddle_fixtures()
MISALIGNED = E.misaligned_fixtures()
SPECIAL = E.special_fixtures()


def cases(fixtures):
    """(loop, fixture) for every loop that takes the fixture: a masked one is the _auto form, which clean.hip has"""
    out = [(loop, f) for f in fixtures for loop in E.LOOPS if f.mask is None or loop == "clean"]
    return dict(argnames="loop,f", argvalues=out, ids=[f"{loop}-{f.name}" for loop, f in out])


@functools.lru_cache(maxsize=None)
def want(loop, f):
    """the restatement's result: computed once per (loop, fixture), never changed"""
    out = E.reference(loop, f)
    for a in out:
        a.setflags(write=False)
    return out


def place(arr, o):
    """(buffer, view): a device buffer of sentinels four cells longer than arr, and arr in it from cell o <= 3 on"""
    import torch
    flat = to_dev(np.ascontiguousarray(arr).ravel())
    fill = SENTINEL if flat.dtype == torch.float64 else 7
    buf = torch.full((flat.numel() + 4,), fill, dtype=flat.dtype, device=flat.device)
    buf[o:o + flat.numel()].copy_(flat)
    return buf, buf[o:o + flat.numel()].view(arr.shape)


def guards_hold(buf, o, n):
    b = host(buf)
    fill = SENTINEL if b.dtype == np.float64 else 7
    return bool((b[:o] == fill).all() and (b[o + n:] == fill).all())


def run_dev(ctx, loop, f, offs=(0, 0, 0), mask_off=1):
    """(model, residual, stats) of the device form; residual, PSF and model start offs cells into buffers of their own
    (a plain torch allocation is 256-byte aligned, so an odd offset is a base 8 bytes off), the mask mask_off bytes.  The
    cells either side of every array are sentinels, and the PSF and the mask are read only: all that is asserted here."""
    N = f.N
    shape = (1, N, N) if loop == "mf1" else (N, N)
    psf, res = E.exact_psf(N).copy().reshape(shape), E.residual_of(f).reshape(shape)
    (rb, rv), (pb, pv), (mb, mv) = place(res, offs[0]), place(psf, offs[1]), place(np.zeros(shape), offs[2])
    kw = dict(gain=f.gain, threshold=0.0, niter=f.niter, border=f.border, patch=f.patch)
    if loop == "clean":
        mask = E.mask_of(f)
        kb, kv = place(mask, mask_off) if mask is not None else (None, None)
        m, r, s = ctx.clean(rv, pv, model=mv, mask=kv, **kw)
        if mask is not None:
            assert guards_hold(kb, mask_off, N * N) and np.array_equal(host(kv), mask), f"{f.name}: the mask was written"
    elif loop == "ms0":
        m, r, s = ctx.msclean(rv, pv, [0.0], [1.0], model=mv, **kw)
    else:
        m, r, s = ctx.mfclean(rv, pv, models=mv, **kw)
    assert m is mv and r is rv
    out = host(m).reshape(N, N), host(r).reshape(N, N), host(s)
    for what, buf, o in (("residual", rb, offs[0]), ("psf", pb, offs[1]), ("model", mb, offs[2])):
        assert guards_hold(buf, o, N * N), f"{loop} {f.name} offsets {offs}: a cell next to the {what} was written"
    assert np.array_equal(host(pv), psf), f"{loop} {f.name}: the PSF was written"
    return out


def assert_bits(got, ref, what):
    for name, g, w in zip(("model", "residual", "stats"), got, ref):
        if not E.same_bits(g, w):
            g, w = np.asarray(g).ravel(), np.asarray(w, dtype=np.float64).ravel()
            bad = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))) if g.shape == w.shape else []
            first = [(int(i), g[i], w[i]) for i in bad[:4]]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} cells, first {first};"
                                 f" stats {got[2]} against {np.asarray(ref[2], dtype=np.float64)}")


@pytest.mark.parametrize(**cases(TIES))
def test_ties_go_to_the_lowest_flat_index(ctx, loop, f):
    """Sections 1 and 2: equal maxima in one slot, in two lanes, in two trips of a wave, in two waves, in two table
    entries, +3 against -3, a constant image inside a border and under a mask.  Bit for bit."""
    assert_bits(run_dev(ctx, loop, f), want(loop, f), f"{loop} {f.name}")


@pytest.mark.parametrize("loop", E.LOOPS)
def test_more_tiles_than_the_pick_kernel_has_threads(ctx, loop):
    """N = 2049, 2193 tiles: five cells stay tied over 12 picks (10 of them exact ties) - in table entries one pick
    thread takes on its first and second trip (88, 1112), on its first and third (144 and 2192, the 1 x 1 corner tile)
    and in another wave (700).  Bit for bit.  The restatement takes about 3 s per loop; the device a fraction of that."""
    f = E.big_fixture()
    assert_bits(run_dev(ctx, loop, f), want(loop, f), f"{loop} {f.name}")


@pytest.mark.parametrize(**cases(RIM))
def test_components_on_the_rim_and_small_images(ctx, loop, f):
    """Section 3: corners and edge midpoints, every patch and border, N from 1 to 257; regions across four tiles, from a
    tile's first cell and from its last.  Bit for bit."""
    assert_bits(run_dev(ctx, loop, f), want(loop, f), f"{loop} {f.name}")


@pytest.mark.parametrize(**cases(MISALIGNED))
def test_bases_eight_bytes_off(ctx, loop, f):
    """Section 4: residual, PSF and model each at an even or an odd cell of its buffer, all eight combinations (and the
    mask at byte 1 and byte 3): the aligned run's bits, the restatement's bits, and no store outside the arrays
    (run_dev asserts the sentinels)."""
    ref = want(loop, f)
    aligned = run_dev(ctx, loop, f, (0, 0, 0), 0)
    assert_bits(aligned, ref, f"{loop} {f.name}, the aligned run against the restatement")
    for o in range(8):
        offs = (o & 1, (o >> 1) & 1, (o >> 2) & 1)
        for mask_off in ((1, 3) if f.mask is not None else (0,)):
            got = run_dev(ctx, loop, f, offs, mask_off)
            assert_bits(got, aligned, f"{loop} {f.name} offsets {offs} mask {mask_off} against the aligned run")
            assert_bits(got, ref, f"{loop} {f.name} offsets {offs} mask {mask_off} against the restatement")


@pytest.mark.parametrize(**cases(SPECIAL))
def test_special_values(ctx, loop, f):
    """Section 5, one iteration each: -0.0 as the only cell that is not NaN, a denormal peak, +inf and -inf tied, NaN all
    around the border.  The restatement's numbers, its NaN pattern and the sign of its zeros."""
    assert_bits(run_dev(ctx, loop, f), want(loop, f), f"{loop} {f.name}")


SCALE_TIES = E.scale_tie_fixtures()


@pytest.mark.parametrize("f", SCALE_TIES, ids=[f.name for f in SCALE_TIES])
def test_a_tie_between_scales_goes_to_the_lowest_scale(ctx, f):
    """Section 6: scales = [0, 1] with biases [1, 1].  The scale 1 has the one tap 1.0, so both scales hold the same
    numbers and every pick ties between them: all components are of scale 0.  Exact, so bit for bit."""
    N = f.N
    (rb, rv), (pb, pv), (mb, mv) = (place(a, 0) for a in (E.residual_of(f), np.array(E.exact_psf(N)), np.zeros((N, N))))
    m, r, s = ctx.msclean(rv, pv, list(E.SCALE_TIE["scales"]), list(E.SCALE_TIE["bias"]), model=mv, gain=f.gain,
                          threshold=0.0, niter=f.niter, border=f.border, patch=f.patch)
    got = host(m), host(r), host(s)
    assert got[2][3] == 0 and got[2][6] == f.niter and got[2][7] == 0, got[2]
    assert_bits(got, E.scale_tie_reference(f), f"scale tie {f.name}")
    assert all(guards_hold(b, 0, N * N) for b in (rb, pb, mb))


# ---- the wide forms -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_want(w):
    return E.wide_reference(w)


def run_wide(ctx, w, offs=(0, 0, 0)):
    """(model, residual, stats) and the three buffers' guards, as run_dev"""
    psf, res = E.wide_inputs(w)
    n = res.size
    (rb, rv), (pb, pv), (mb, mv) = place(res, offs[0]), place(psf, offs[1]), place(np.zeros_like(res), offs[2])
    kw = dict(gain=w.gain, threshold=0.0, niter=w.niter, border=w.border, patch=w.patch)
    if w.kind == "ms":
        m, r, s = ctx.msclean(rv, pv, list(w.scales), list(w.bias), model=mv, **kw)
    else:
        m, r, s = ctx.mfclean(rv, pv, models=mv, **kw)
    assert m is mv and r is rv
    out = host(m), host(r), host(s)
    for what, buf, o, cells in (("residual", rb, offs[0], n), ("psf", pb, offs[1], psf.size), ("model", mb, offs[2], n)):
        assert guards_hold(buf, o, cells), f"{w.name} offsets {offs}: a cell next to the {what} was written"
    assert np.array_equal(host(pv), psf), f"{w.name}: the PSF was written"
    return out


def compare_wide(w, got, what=None):
    ref = wide_want(w)
    peak = np.abs(E.wide_inputs(w)[1]).max()
    (compare_ms if w.kind == "ms" else compare_mf)(got, ref, peak, what or w.name)
    if w.kind == "ms":
        assert np.array_equal(got[2][6:], ref[2][6:]), (w.name, got[2], ref[2])


WIDE_TIES, WIDE_RIM, WIDE_MIS = E.wide_tie_fixtures(), E.wide_rim_fixtures(), E.wide_misaligned_fixtures()
BIG_WIDE = E.wide_big_fixtures()
wids = lambda ws: [w.name for w in ws]  # noqa: E731


@pytest.mark.parametrize("w", WIDE_TIES, ids=wids(WIDE_TIES))
def test_wide_ties_by_translation(ctx, w):
    """Identical stamps in rows r and r + 4 of a tile, rows 4 and 1, a later table entry with the lower index, two tile
    rows; scales [0, 2] and [0, 32] (radius 31), T = 2 and 3: picks 0 and 2 are exact ties."""
    compare_wide(w, run_wide(ctx, w))


@pytest.mark.parametrize("w", BIG_WIDE, ids=wids(BIG_WIDE))
def test_wide_ties_with_more_tiles_than_pick_threads(ctx, w):
    """N = 2049, patch 32, stamps in entries 88, 700 and 1112.  The restatement's run takes about 4 s for msclean with
    scales [0, 2] at niter = 3 (picks 0 and 1 tie) and about 3 s for mfclean with T = 2 at niter = 5 (picks 0, 1, 3
    and 4 tie), timed on the host; one more pick costs about 0.5 s."""
    compare_wide(w, run_wide(ctx, w))


@pytest.mark.parametrize("w", WIDE_RIM, ids=wids(WIDE_RIM))
def test_wide_components_on_the_rim_and_small_images(ctx, w):
    """N in {1, 2, 3, 17, 129}, corners and edge midpoints, the whole PSF and patch 1"""
    compare_wide(w, run_wide(ctx, w))


@pytest.mark.parametrize("w", WIDE_MIS, ids=wids(WIDE_MIS))
def test_wide_planes_eight_bytes_off(ctx, w):
    """Even N: plane 0 of the residual, PSF and model stacks at an even or odd cell of its buffer, all eight
    combinations.  The aligned run's bits (the arithmetic does not depend on how a slot is loaded), the restatement
    within the tolerance, the sentinels either side untouched (run_wide asserts them)."""
    aligned = run_wide(ctx, w)
    compare_wide(w, aligned, f"{w.name} aligned")
    for o in range(1, 8):
        offs = (o & 1, (o >> 1) & 1, (o >> 2) & 1)
        got = run_wide(ctx, w, offs)
        assert_bits(got, aligned, f"{w.name} offsets {offs} against the aligned run")
