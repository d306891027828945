"""Continuum subtraction on the device (gridhip_contsub[_dev]) against the numpy restatement tests/contsub_ref.py.  Every
comparison with the restatement is bit for bit - out, coeffs, rowinfo, codes, stats (NaN in the same places): every
floating-point result belongs to one lane and one fixed order of rounded operations, so there is no tolerance to state.
The shapes are the smallest at which each path can go wrong: rows either side of a work-group of both kernels, channels
either side of the staged chunk and of the block the channel-outermost kernel loads ahead, one channel, one row.

Not tested: that a call without codes and without clip rounds draws no n-byte block from the context's pool - the
context exposes no pool statistics, and none is added for a test."""
import ctypes as C

import numpy as np
import pytest

import contsub_ref as R
from test_contsub_host import CLIP_SEED
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

c128, f64, u8 = np.complex128, np.float64, np.uint8
NAN, INF = np.nan, np.inf
NAMES = ("out", "coeffs", "info", "codes", "stats")


def dev(x):
    return None if x is None else to_dev(x)


def run(ctx, data, x, mask=None, weights=None, form="dev", axis=-1, in_place=False, **kw):
    """data [R][C] -> (out, coeffs, info, codes, stats) as numpy arrays in the [R][...] arrangement, by the device form
    (torch tensors) or the host form, with the cube handed over along `axis` ([R][C], or [C][R] for axis 0)"""
    turn = (lambda a: None if a is None else np.ascontiguousarray(np.asarray(a).T)) if axis == 0 else (lambda a: a)
    d, w = turn(np.ascontiguousarray(data)), turn(weights)
    m = None if mask is None else np.asarray(mask)
    if form == "host":
        d = d.copy() if in_place else d
        got = ctx.contsub(d, x, m, w, axis=axis, codes=True, out=d if in_place else None, **kw)
    else:
        dd = dev(d)
        got = ctx.contsub(dd, dev(np.asarray(x, dtype=f64)), dev(m), dev(w), axis=axis, codes=True, out=dd if in_place else None, **kw)
        assert not in_place or got[0] is dd
        got = tuple(host(t) for t in got)
    return tuple(turn(a) for a in got[:4]) + (got[4],)


def same(what, got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, not {w.dtype}{w.shape}"
        if name == "codes":
            assert np.array_equal(g, w), f"{what}: codes differ at {np.argwhere(g != w)[:8].tolist()}: {g[g != w][:8]} for {w[g != w][:8]}"
        else:
            gc, wc = R.canon(g), R.canon(w)
            assert R.same_bits(gc, wc), f"{what}: {name} differs: {first_difference(gc, wc)}"


def first_difference(a, b):
    """(flat index of the first double that differs, got, wanted, how many differ)"""
    a, b = np.ascontiguousarray(a).view(np.uint64).ravel(), np.ascontiguousarray(b).view(np.uint64).ravel()
    k = np.flatnonzero(a != b)
    return None if k.size == 0 else (int(k[0]), a.view(f64)[k[0]], b.view(f64)[k[0]], int(k.size))


def both(ctx, what, data, x, mask=None, weights=None, forms=("dev",), axes=(-1, 0), **kw):
    want = R.contsub(data, x, mask, weights, **kw)
    got = None
    for axis in axes:
        for form in forms:
            got = run(ctx, data, x, mask, weights, form=form, axis=axis, **kw)
            same(f"{what} [{form}, axis {axis}]", got, want)
    return got, want


def spectra(rng, Rr, Cc, cplx=True, noise=0.05, holes=True):
    """Rr rows of a cubic continuum plus noise over Cc channels, weights in [0.5, 2] with a tenth of them zero, a mask with a
    hole where the row is long enough -> data [R][C], x, mask, weights"""
    x = np.linspace(-1.0, 1.0, Cc) if Cc > 1 else np.zeros(1)
    a = rng.normal(size=(Rr, 4)) + 1j * rng.normal(size=(Rr, 4))
    data = a @ np.stack([np.ones(Cc), x, 2 * x * x - 1, 4 * x ** 3 - 3 * x]) + noise * (rng.normal(size=(Rr, Cc)) + 1j * rng.normal(size=(Rr, Cc)))
    data = np.ascontiguousarray(data if cplx else data.real)
    w = rng.uniform(0.5, 2.0, (Rr, Cc))
    mask = np.ones(Cc, dtype=bool)
    if holes:
        w[rng.random((Rr, Cc)) < 0.1] = 0.0
        if Cc > 4:
            mask[Cc // 2:Cc // 2 + max(1, Cc // 8)] = False
    return data, x, mask, w


@pytest.fixture(scope="module")
def tile():
    import gridhip
    return gridhip.contsub_tile()


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def edge_case(ctx, Rr, Cc, k):
    """one shape: the degree, the number of components, the mode and whether rounds run all turn with k"""
    rng = np.random.default_rng(1000 * Rr + Cc)
    D, cplx, mode = k % 4, bool((k // 2) % 2), ("subtract", "model")[k % 2]
    data, x, mask, w = spectra(rng, Rr, Cc, cplx)
    if Cc > 8:
        data[:, 1] += 3.0  # something to clip
    kw = dict(degree=D, mode=mode, nsigma=2.5 if k % 3 else 0.0, niter=k % 3)
    both(ctx, f"R = {Rr}, C = {Cc}, {kw}, complex {cplx}", data, x, mask, w, **kw)
    both(ctx, f"R = {Rr}, C = {Cc}, degree {3 - D}, bare, complex {not cplx}", spectra(rng, Rr, Cc, not cplx)[0], x, degree=3 - D)


def test_rows_either_side_of_a_work_group(ctx, tile):
    rows, chunk = tile
    Rs, Cs = [1, rows - 1, rows, rows + 1, 2 * rows + 1], [1, 2, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    k = 0
    for i, Rr in enumerate(Rs):
        for Cc in (Cs[(2 * i) % 8], Cs[(2 * i + 5) % 8]):
            edge_case(ctx, Rr, Cc, k)
            k += 1
    # the channel-outermost kernel's work-group is 256 rows
    for Rr, Cc in ((255, chunk + 1), (256, 5), (257, 2 * chunk + 3), (513, 3)):
        edge_case(ctx, Rr, Cc, k)
        k += 1


def test_channels_either_side_of_a_chunk(ctx, tile):
    rows, chunk = tile
    Rs, Cs = [1, rows - 1, rows, rows + 1, 2 * rows + 1], [1, 2, 3, 4, 5, 7, 8, 9, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 3]
    k = 5
    for j, Cc in enumerate(Cs):
        for Rr in (Rs[j % 5], Rs[(j + 2) % 5]):
            edge_case(ctx, Rr, Cc, k)
            k += 1


def test_every_instantiation(ctx, tile):
    """degrees 0 to 3 x real and complex x both layouts x both modes, with rounds, on one shape that is no multiple of anything"""
    rows, chunk = tile
    rng = np.random.default_rng(7)
    for cplx in (False, True):
        data, x, mask, w = spectra(rng, rows + 3, 2 * chunk + 5, cplx)
        data[:, 3] += 2.0
        for D in range(4):
            for mode in ("subtract", "model"):
                (out, co, info, codes, stats), _ = both(ctx, f"degree {D}, {mode}, complex {cplx}", data, x, mask, w, degree=D, mode=mode,
                                                        nsigma=3.0, niter=2)
                assert stats[0] == rows + 3 and stats[1] == rows + 3 and (info[:, 0] == D).all() and stats[5] > 0


def test_layout_equality(ctx, tile):
    """the same cube as [R][C] and as [C][R]: the same bits in all five outputs after the transposition of coeffs and info,
    the two results compared with each other"""
    rows, chunk = tile
    rng = np.random.default_rng(8)
    for Rr, Cc, cplx in ((2 * rows + 1, 2 * chunk + 3, True), (257, chunk + 1, False)):
        data, x, mask, w = spectra(rng, Rr, Cc, cplx, noise=0.2)
        data[:, 2] += 4.0
        a = run(ctx, data, x, mask, w, axis=-1, degree=3, nsigma=2.5, niter=4)
        b = run(ctx, data, x, mask, w, axis=0, degree=3, nsigma=2.5, niter=4)
        same(f"R = {Rr}, C = {Cc}: axis 0 against axis -1", b, a)
        assert a[4][5] > 0 and (a[3] == 17).any(), "a second round clipped something"


# ---- forms, reruns, the graph -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_want(tile):
    """the host test's clip case at R = 2 rows + 1, and one more row that round 0 clips and round 1 leaves alone"""
    rows, _ = tile
    data, x, line = R.clip_case(CLIP_SEED, R=2 * rows + 1)
    extra = (0.5 + 0.25j) * (1.0 + x) + 0.01 * np.where(np.arange(x.size) % 2, 1.0, -1.0)
    extra[40] += 3.0
    data = np.ascontiguousarray(np.vstack([data, extra[None, :]]))
    return data, x, line, R.contsub(data, x, degree=3, nsigma=3.0, niter=4)


def test_clip(ctx, clip_want):
    data, x, line, want = clip_want
    for axis in (-1, 0):
        got = run(ctx, data, x, axis=axis, degree=3, nsigma=3.0, niter=4)
        same(f"clip, axis {axis}", got, want)
    codes, info = got[3], got[2]
    assert (codes[:-1][line] >= 16).all()
    assert codes[-1, 40] == 16 and (codes[-1] == 16).sum() == 1 and not (codes[-1] == 17).any() and info[-1, 2] == 1


def test_fixed_bits(ctx, clip_want):
    """the host form, the _dev form, a second run, and out passed as data against a separate out"""
    data, x, _, want = clip_want
    kw = dict(degree=3, nsigma=3.0, niter=4)
    for axis in (-1, 0):
        for form in ("host", "dev"):
            same(f"{form}, axis {axis}", run(ctx, data, x, form=form, axis=axis, **kw), want)
            same(f"{form}, axis {axis}, again", run(ctx, data, x, form=form, axis=axis, **kw), want)
            same(f"{form}, axis {axis}, in place", run(ctx, data, x, form=form, axis=axis, in_place=True, **kw), want)
    rng = np.random.default_rng(9)
    d2, x2, mask, w = spectra(rng, 70, 21, False)
    for mode in ("subtract", "model"):
        want2 = R.contsub(d2, x2, mask, w, degree=2, mode=mode)
        for axis in (-1, 0):
            same(f"real, {mode}, axis {axis}, in place", run(ctx, d2, x2, mask, w, axis=axis, in_place=True, degree=2, mode=mode), want2)


def test_a_repeated_call_takes_no_memory(ctx, clip_want):
    import torch
    data, x, _, want = clip_want
    dd, dx = dev(data), dev(x)
    kw = dict(degree=3, nsigma=3.0, niter=4)
    out = torch.empty_like(dd)
    ctx.contsub(dd, dx, out=out, **kw)  # (the pool then holds the table and the call's own bytes, torch's cache the outputs)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    got = ctx.contsub(dd, dx, out=out, **kw)
    torch.cuda.synchronize()
    assert got[0] is out and got[3] is None and torch.cuda.mem_get_info()[0] == free
    assert R.same_bits(host(out), want[0]) and bool((dd == dev(data)).all())


def test_a_captured_call_replays_to_the_eager_result(ctx, clip_want):
    import torch
    data, x, _, want = clip_want
    for axis in (-1, 0):
        dd = dev(data if axis == -1 else np.ascontiguousarray(data.T))
        dx, out = dev(x), torch.empty_like(dd)
        kw = dict(axis=axis, degree=3, nsigma=3.0, niter=4, codes=True, out=out)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds the call's scratch
            ctx.contsub(dd, dx, **kw)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
            res = ctx.contsub(dd, dx, **kw)
        torch.cuda.synchronize()
        for _ in range(2):
            for t in res:
                t.fill_(7)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            got = [host(t) for t in res]
            if axis == 0:
                got = [np.ascontiguousarray(a.T) for a in got[:4]] + [got[4]]
            same(f"replay, axis {axis}", got, want)


# ---- classes -----------------------------------------------------------------------------------------------------------------
def test_classes(ctx):
    """zero, negative, NaN and Inf weights, NaN and Inf values, a channel whose x is not finite (a NaN column in out, every
    other column as without it), and masks that leave D, D + 1 and 0 channels: reduced degree, full degree, none"""
    rng = np.random.default_rng(10)
    Rr, Cc, D = 70, 37, 2
    data, x, mask, w = spectra(rng, Rr, Cc, True, holes=False)
    w[0, 0], w[1, 1], w[2, 2], w[3, 3], w[4, :] = 0.0, -1.0, NAN, INF, 0.0
    data[5, 5], data[6, 6], data[7, 7], data[8, 8] = NAN, INF, 1j * NAN, 1 - 1j * INF
    w[9, 9], data[9, 9] = 0.0, NAN      # the first class that applies: 1
    xn = x.copy()
    xn[11], xn[30] = NAN, INF
    mask[20] = False
    data[10, 11] = NAN                   # class 3 before class 2
    (out, co, info, codes, stats), want = both(ctx, "classes", data, xn, mask, w, forms=("dev", "host"), degree=D)
    assert codes[0, 0] == codes[1, 1] == codes[2, 2] == codes[3, 3] == 1 and (codes[4] == 1).all() and codes[9, 9] == 1
    assert codes[5, 5] == codes[6, 6] == codes[7, 7] == codes[8, 8] == codes[10, 11] == 3
    assert (np.delete(codes[:, [11, 30, 20]], [4, 10], axis=0) == 2).all()
    assert np.isnan(out[:, [11, 30]]).all() and info[4].tolist()[:3] == [-1, 0, 0] and np.isnan(info[4, 3])
    assert (codes == 2).sum() + stats[4:].sum() == Rr * Cc and stats.tolist()[:4] == [Rr, Rr - 1, 0, 1] and stats[5] == 0
    # every other column is as it is without those two channels
    keep = np.ones(Cc, dtype=bool)
    keep[[11, 30]] = False
    sub = R.contsub(np.ascontiguousarray(data[:, keep]), x[keep], mask[keep], np.ascontiguousarray(w[:, keep]), degree=D)
    assert R.same_bits(R.canon(out[:, keep]), R.canon(sub[0])) and R.same_bits(co, sub[1])
    # a NaN value in a channel with a NaN coordinate stays NaN; out == data is as a separate out
    same("classes, in place", run(ctx, data, xn, mask, w, in_place=True, degree=D), want)
    # masks that leave D, D + 1 and 0 channels
    for left, deg in ((D, D - 1), (D + 1, D), (0, -1)):
        m = np.zeros(Cc, dtype=bool)
        m[[3, 17, 33][:left]] = True
        (out, co, info, codes, stats), _ = both(ctx, f"{left} channels", data, x, m, None, degree=D)
        rows_ok = np.isfinite(data[:, m]).all(axis=1)
        assert (info[rows_ok, 0] == deg).all() and stats[1] == (rows_ok.sum() if deg == D else 0)
        assert (codes == 2).sum() + stats[4:].sum() == Rr * Cc
        if left == 0:
            assert R.same_bits(R.canon(out), R.canon(data)) and stats[3] == Rr and (co == 0).all()


def test_one_row_one_channel_and_a_degenerate_coordinate(ctx):
    both(ctx, "1 x 1", np.array([[2.5 - 1j]]), np.zeros(1), degree=3, forms=("dev", "host"))
    both(ctx, "1 x 1 real, flagged", np.array([[2.5]]), np.zeros(1), None, np.zeros((1, 1)), degree=0, mode="model")
    rng = np.random.default_rng(11)
    data = rng.normal(size=(5, 9))
    (out, co, info, codes, stats), _ = both(ctx, "all channels at x = 0", data, np.zeros(9), degree=3, nsigma=1.0, niter=4)
    assert (info[:, 0] == 0).all() and stats[2] == 5


def test_samples_past_2_31(ctx):
    """2^20 + 3 spectra of 1024 complex channels: the doubles of the last rows lie past index 2^31 (17 GB, made and kept on
    the device).  Rows are independent, so the first and the last rows of the large call must carry the bits of a call
    on those rows alone - in both layouts."""
    import torch
    Rr, Cc, edge = (1 << 20) + 3, 1024, 67
    g = torch.Generator(device="cuda:0").manual_seed(3)
    flat = torch.randn(Rr * Cc * 2, dtype=torch.float64, device="cuda:0", generator=g)
    x = torch.linspace(-1.0, 1.0, Cc, dtype=torch.float64, device="cuda:0")
    kw = dict(degree=3, nsigma=2.5, niter=2, codes=True)
    for axis in (-1, 0):
        d = torch.view_as_complex(flat.view(-1, 2)).view((Rr, Cc) if axis == -1 else (Cc, Rr))
        rows_of = (lambda t, s: t[s]) if axis == -1 else (lambda t, s: t[:, s])  # noqa: E731
        big = ctx.contsub(d, x, axis=axis, **kw)
        for s in (slice(0, edge), slice(Rr - edge, Rr)):
            small = ctx.contsub(rows_of(d, s).contiguous(), x, axis=axis, **kw)
            for name, b, sm in zip(NAMES[:4], big, small):
                assert R.same_bits(host(rows_of(b, s).contiguous()), host(sm)), f"axis {axis}, rows {s}: {name}"
            assert float(small[4][5]) > 0
        assert big[4].tolist()[:2] == [Rr, Rr]
        del big, small, d
    del flat
    torch.cuda.empty_cache()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """Every rule of the header through the C ABI on device memory, and the outputs as they were given."""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    Rr, Cc, D = 3, 5, 2
    n = Rr * Cc
    full = lambda m, val, dt: torch.full((m,), val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(x=full(2 * Cc, 0.5, torch.float64), m=full(2 * Cc, 1, torch.uint8), d=full(2 * n, 2 + 1j, torch.complex128),
             w=full(2 * n, 1.5, torch.float64), o=full(n, 4 - 1j, torch.complex128), c=full(Rr * (D + 1), 7 + 0j, torch.complex128),
             r=full(Rr * 4, 5.0, torch.float64), k=full(n, 9, torch.uint8), s=full(8, 6.0, torch.float64))
    p = {key: C.c_void_p(v.data_ptr()) for key, v in t.items()}
    h = ctx._h

    def cs(R=Rr, C=Cc, layout=0, ncomp=2, degree=D, mode=0, x=p["x"], m=p["m"], d=p["d"], w=p["w"], nsigma=3.0, niter=2, o=p["o"],
           c=p["c"], r=p["r"], k=p["k"], s=p["s"]):
        return lib.gridhip_contsub_dev(h, R, C, layout, ncomp, degree, mode, x, m, d, w, nsigma, niter, o, c, r, k, s)

    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    bad = [cs(d=None), cs(x=None), cs(o=None), cs(R=0), cs(R=-1), cs(C=0), cs(layout=2), cs(layout=-1), cs(mode=2), cs(mode=-1),
           cs(ncomp=0), cs(ncomp=3), cs(degree=-1), cs(degree=4), cs(nsigma=-0.5), cs(nsigma=NAN), cs(nsigma=INF), cs(niter=-1),
           cs(niter=5),
           # an output over an input
           cs(o=at("d", 16)), cs(o=p["w"]), cs(o=p["x"]), cs(o=p["m"]), cs(c=p["d"]), cs(c=p["w"]), cs(r=p["d"]), cs(r=at("x", 8)),
           cs(k=p["d"]), cs(k=p["m"]), cs(k=at("w", 8 * n - 1)), cs(s=p["d"]), cs(s=at("w", 8)), cs(s=p["x"]),
           # an output over another output
           cs(c=p["o"]), cs(c=at("o", 16 * n - 8)), cs(r=p["o"]), cs(k=p["o"]), cs(s=p["o"]), cs(r=p["c"]), cs(k=p["c"]),
           cs(s=at("c", 16 * Rr * (D + 1) - 8)), cs(k=p["r"]), cs(s=p["r"]), cs(s=p["k"])]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), bad
    big = [cs(C=4097), cs(R=1 << 31), cs(R=1 << 40, C=4096)]
    assert big == [_lib.EUNSUPPORTED] * len(big), big
    assert cs(C=4097, degree=4) == _lib.EINVAL
    assert lib.gridhip_contsub_dev(None, Rr, Cc, 0, 2, D, 0, p["x"], p["m"], p["d"], p["w"], 3.0, 2, p["o"], p["c"], p["r"], p["k"],
                                   p["s"]) == _lib.EINVAL
    torch.cuda.synchronize()
    for key, val in (("x", 0.5), ("m", 1), ("d", 2 + 1j), ("w", 1.5), ("o", 4 - 1j), ("c", 7 + 0j), ("r", 5.0), ("k", 9), ("s", 6.0)):
        assert bool((t[key] == val).all()), key
    # and the valid corners next to them: no mask, no weights, no optional output, out == data, an output that ends where
    # an input begins
    assert cs(m=None, w=None, c=None, r=None, k=None, s=None) == 0 and cs(o=p["d"], niter=0) == 0
    assert cs(o=at("d", 16 * n), layout=1, nsigma=0.0) == 0
    ctx.synchronize()
