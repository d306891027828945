"""Local background and noise maps on the device (gridhip_noise_map[_dev], Context.noise_map, automask_local) against the
numpy restatement of include/gridhip.h's definition (tests/noisemap_ref.py).

Every value is an order statistic, a count or a fixed sequence of rounded operations: every comparison is bit for bit,
the sign of zeros and the placement of NaNs included (`same`)."""
import ctypes as C

import numpy as np
import pytest

import noise_ref
import noisemap_ref as ref
from test_noisemap_host import ramp_image

pytestmark = pytest.mark.gpu

NAMES = ("background", "rms", "out", "nodes", "stats")
# N, border, step, half, min_count: the smallest shapes at which each path can go wrong
SHAPES = {
    "one cell": (1, 0, 16, 1, 1),                   # G = 1
    "M below step": (7, 0, 16, 3, 3),               # one node, its centre clamped
    "clipped windows": (37, 3, 5, 4, 6),            # windows clipped on all four sides, cells beyond the last centre
    "full window": (150, 0, 40, 64, 16),            # 129 x 129 keys: the 133 KB window, larger than the spacing
    "tiny nodes": (130, 0, 1, 1, 3),                # 16 900 nodes of 9 cells
    "usual": (257, 0, 16, 32, 16),
}


def same(a, b):
    """the same bits: NaNs in the same places, and everywhere else equal values of equal sign (+0.0 is not -0.0).  The sign
    and payload of a NaN that arithmetic produces (Inf - Inf, NaN / x) are not IEEE 754's to define and differ between
    processors, so a NaN is compared by its place alone."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return np.array_equal(a[ok], b[ok]) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def to_dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def patterns(N, seed):
    """test_gpu_noise.py's set, and a three-valued integer image (ties in the median and at the clip limit)"""
    rng = np.random.default_rng(seed)
    n = N * N
    out = {"gaussian": rng.normal(size=n), "equal": np.full(n, 0.3)}
    out["two values"] = np.where(np.arange(n) % 2 == 0, -1.5, 2.5)
    out["zeros denormals huge"] = rng.choice([0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e308, -1e308, 1.7e308, 3.0, -3.0], n)
    low = np.full(n, 1.0).view(np.uint64) + rng.integers(0, 7, n).astype(np.uint64)
    out["lowest digit"] = low.view(np.float64)
    bad = rng.normal(size=n)
    bad[rng.integers(0, n, max(1, n // 9))] = np.nan
    bad[rng.integers(0, n, max(1, n // 11))] = np.inf
    bad[rng.integers(0, n, max(1, n // 13))] = -np.inf
    out["nan and inf"] = bad
    out["three values"] = rng.integers(0, 3, n).astype(np.float64)
    return {k: v.reshape(N, N) for k, v in out.items()}


def compare(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
        else:
            g = host(g) if hasattr(g, "cpu") else g
            assert same(g, w), f"{what}: {name} differs at {np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:4].tolist()}"


def check(ctx, img, mask=None, what="", **kw):
    want = ref.noise_map(img, mask, **kw)
    got = ctx.noise_map(to_dev(img), to_dev(mask), **kw)
    compare(got, want, what)
    return want


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bit_for_bit(ctx, shape):
    N, border, step, half, min_count = SHAPES[shape]
    rng = np.random.default_rng(N)
    kw = dict(border=border, step=step, half=half, min_count=min_count)
    pats = patterns(N, N)
    tiny = shape == "tiny nodes"  # (the restatement walks 16 900 windows per call: two calls)
    if tiny:
        pats = {k: pats[k] for k in ("gaussian", "three values")}
    parity = set()
    for name, img in pats.items():
        masks = [(None, False)]
        if N > 4:
            masks += [(rng.random((N, N)) < 0.6, False), ((rng.random((N, N)) < 0.3).astype(np.uint8) * 3, True)]
        if tiny:
            masks = masks[:1] if name == "gaussian" else masks[1:2]
        for mask, exclude in masks:
            want = check(ctx, img, mask, f"{shape} {name} mask {mask is not None} exclude {exclude}", exclude=exclude,
                         mode="snr", **kw)
            parity |= {int(v) % 2 for v in want[3][2].ravel() if v > 0}
    if N > 4 and not tiny:
        assert parity == {0, 1}, "windows of even and of odd counts"
        # ties at the clip limit: with kappa = 1 / 1.4826 and MAD = 1, d_k = 1 is at L or just above it
        check(ctx, pats["three values"], None, f"{shape} three values at the limit", kappa=1.0 / 1.4826, mode="subtract", **kw)


def test_masks_and_invalid_nodes(ctx):
    N, border, step, half, min_count = SHAPES["clipped windows"]
    kw = dict(border=border, step=step, half=half, min_count=min_count, mode="snr")
    rng = np.random.default_rng(5)
    img = rng.normal(size=(N, N))
    # a mask that empties some nodes, leaves min_count - 1 cells to node (2, 2) and min_count to node (4, 4)
    mask = np.zeros((N, N), dtype=np.uint8)
    mask[11:16, 11] = 1
    mask[21:27, 29] = 1
    want = check(ctx, img, mask, "counted mask", **kw)
    n_used = want[3][2]
    assert n_used[2, 2] == min_count - 1 and np.isnan(want[3][0][2, 2])
    assert n_used[4, 4] == min_count and np.isfinite(want[3][0][4, 4]) and np.isfinite(want[3][1][4, 4])
    assert (n_used == 0).any() and 0 < want[4][1] < n_used.size
    # the same cells shut out instead
    check(ctx, img, mask, "counted mask, excluded", exclude=True, **kw)
    # masks that empty every node, both ways round: every map cell is NaN
    for m, exclude in ((np.zeros((N, N), dtype=np.uint8), False), (np.full((N, N), 7, dtype=np.uint8), True)):
        want = check(ctx, img, m, f"empty exclude {exclude}", exclude=exclude, **kw)
        assert want[4][1] == 0 and want[4][2] == 0 and np.isnan(want[4][3]) and np.isnan(want[4][4])
        assert np.isnan(want[0]).all() and np.isnan(want[1]).all() and np.isnan(want[2]).all()
        assert want[4][5] == (N - 2 * border) ** 2
    # a constant patch over the windows of nodes 2 and 3: a background and no rms there, and around it every branch of lerp
    img[11:25, 11:25] = 0.75
    branches = [0, 0, 0, 0]
    want = ref.noise_map(img, None, branches=branches, **kw)
    assert np.isfinite(want[3][0]).all() and np.isnan(want[3][1][2:4, 2:4]).all()
    assert 4 <= np.count_nonzero(np.isnan(want[3][1])) < want[3][1].size  # (a window that is mostly patch clips down to it)
    assert all(b > 0 for b in branches), f"lerp branches both / only a / only b / neither: {branches}"
    compare(ctx.noise_map(to_dev(img), None, **kw), want, "constant patch")


@pytest.mark.parametrize("nclip", [0, 1, 8])
def test_clip_rounds_on_a_bright_blob(ctx, nclip):
    N = 65
    img = np.random.default_rng(0).normal(size=(N, N))
    y, x = np.mgrid[0:N, 0:N]
    img += 50.0 * np.exp(-((y - N // 2) ** 2 + (x - N // 2) ** 2) / (2.0 * 4.0 ** 2))
    want = check(ctx, img, None, f"blob nclip {nclip}", step=65, half=32, nclip=nclip, mode="subtract")
    assert want[4][6] == {0: 0, 1: 1, 8: 3}[nclip]  # three rounds remove the blob; a fourth drops nothing
    # and on a mesh, where the windows hold more or less of it
    check(ctx, img, None, f"blob mesh nclip {nclip}", step=8, half=12, nclip=nclip, mode="snr")


def raw_call(ctx, dev, N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, wanted, out_is_image=False):
    """the C entry point itself with NULL for the outputs not in `wanted`; -> dict of host arrays"""
    import torch
    G = ref.centres(N, border, step)
    sizes = dict(nodes=(4, len(G), len(G)), background=(N, N), rms=(N, N), out=(N, N), stats=(8,))
    if dev:
        image = to_dev(image)
        mask = to_dev(mask)
        bufs = {k: torch.full(sizes[k], 7.0, dtype=torch.float64, device="cuda:0") for k in wanted}
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        ctx._use_torch_stream()
    else:
        image = np.ascontiguousarray(image).copy()
        bufs = {k: np.full(sizes[k], 7.0) for k in wanted}
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    if out_is_image:
        bufs["out"] = image
    fn = ctx._lib.gridhip_noise_map_dev if dev else ctx._lib.gridhip_noise_map
    rc = fn(ctx._h, N, p(image), p(mask), int(exclude), border, step, half, kappa, nclip, min_count, mode,
            *(p(bufs.get(k)) for k in ("nodes", "background", "rms", "out", "stats")))
    assert rc == 0, ctx._error(rc)
    if dev:
        torch.cuda.synchronize()
    return {k: (host(v) if dev else v) for k, v in bufs.items()}


def test_modes_forms_null_outputs_and_in_place_twice(ctx):
    N, border, step, half, min_count = 61, 2, 7, 9, 10
    rng = np.random.default_rng(11)
    img = rng.normal(size=(N, N)) * np.linspace(1, 3, N)[None, :] + 0.5
    img[5, 6] = np.nan
    img[40, 41] = np.inf
    mask = rng.random((N, N)) < 0.2
    kw = dict(exclude=True, border=border, step=step, half=half, kappa=2.5, nclip=2, min_count=min_count)
    for mode in (None, "subtract", "snr"):
        want = ref.noise_map(img, mask, mode=mode, **kw)
        for rep in range(2):
            compare(ctx.noise_map(img, mask, mode=mode, **kw), want, f"host form mode {mode}")
            compare(ctx.noise_map(to_dev(img), to_dev(mask), mode=mode, **kw), want, f"dev form mode {mode}")
        # maps=False leaves them out and changes nothing else
        got = ctx.noise_map(to_dev(img), to_dev(mask), mode=mode, maps=False, **kw)
        assert got[0] is None and got[1] is None
        compare(got[2:], want[2:], f"no maps mode {mode}")
        if mode is not None:  # out is image, in both forms
            a = img.copy()
            got = ctx.noise_map(a, mask, mode=mode, out=a, **kw)
            assert got[2] is a
            compare(got, want, f"host form in place mode {mode}")
            d = to_dev(img)
            got = ctx.noise_map(d, to_dev(mask), mode=mode, out=d, **kw)
            assert got[2] is d
            compare(got, want, f"dev form in place mode {mode}")
    # NULL combinations of the optional outputs at the C entry point, both forms
    want = dict(zip(NAMES, ref.noise_map(img, mask.astype(np.uint8), mode="snr", **kw)))
    args = (N, img, mask.astype(np.uint8), 1, border, step, half, 2.5, 2, min_count)
    for dev in (False, True):
        for mode, wanted in ((0, ("stats",)), (0, ("nodes", "stats")), (0, ("background", "stats")), (0, ("rms", "stats")),
                             (2, ("out", "stats")), (2, ("rms", "out", "stats")), (2, ("nodes", "background", "out", "stats")),
                             (0, ("out", "stats"))):
            got = raw_call(ctx, dev, *args, mode, wanted)
            for k, v in got.items():
                if k == "out" and mode == 0:
                    assert (v == 7.0).all(), "mode 0 writes no out"
                elif k == "stats" and mode == 0:
                    assert same(v[[0, 1, 2, 3, 4, 6, 7]], want[k][[0, 1, 2, 3, 4, 6, 7]]) and v[5] == 0
                else:
                    assert same(v, want[k]), (dev, mode, wanted, k)
        got = raw_call(ctx, dev, *args, 2, ("stats",), out_is_image=True)
        assert same(got["out"], want["out"]) and same(got["stats"], want["stats"])


@pytest.mark.parametrize("shape", ["clipped windows", "full window", "usual"])
def test_every_histogram_strategy_gives_the_same_bits(ctx, shape):
    N, border, step, half, min_count = SHAPES[shape]
    pats = patterns(N, 3)
    kw = dict(border=border, step=step, half=half, min_count=min_count, mode="snr")
    try:
        for name in ("gaussian", "lowest digit", "zeros denormals huge", "equal"):
            want = ref.noise_map(pats[name], None, **kw)
            d = to_dev(pats[name])
            for strat in range(8):
                ctx.set_option("noisemap_hist", strat)
                compare(ctx.noise_map(d, None, **kw), want, f"{shape} {name} noisemap_hist {strat}")
    finally:
        ctx.set_option("noisemap_hist", 0)


def test_noise_map_and_automask_in_one_graph(ctx):
    import torch
    N = 96
    kw = dict(border=2, step=8, half=12, nclip=2)
    akw = dict(border=2, thr=(4.0, 2.5), nsigma=(0, 0), min_cells=2, grow=1)

    def image(seed):
        rng = np.random.default_rng(seed)
        img = rng.normal(size=(N, N)) * np.linspace(1, 4, N)[:, None]
        img[20:23, 30:33] += 40.0
        img[70:72, 60:63] += 60.0
        return img
    img = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    mask = torch.zeros((N, N), dtype=torch.uint8, device="cuda:0")

    def work(img, mask):
        bg, rms, snr, nodes, nst = ctx.noise_map(img, mode="snr", **kw)
        _, ast = ctx.automask(snr, mask, **akw)
        return bg, rms, snr, nodes, nst, ast
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up on the capture stream: the first calls' allocations
        img.copy_(to_dev(image(0)))
        work(img, mask)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        outs = work(img, mask)
    torch.cuda.synchronize()
    for rep in (1, 2):
        fresh = image(rep)
        img.copy_(to_dev(fresh))
        mask.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = ref.noise_map(fresh, None, mode="snr", **kw)
        compare(outs[:5], want, f"replay {rep}")
        e_mask = torch.zeros_like(mask)
        _, e_ast = ctx.automask(to_dev(want[2]), e_mask, **akw)
        torch.cuda.synchronize()
        assert host(mask).any() and np.array_equal(host(mask), host(e_mask)) and same(host(outs[5]), host(e_ast))
    assert ctx.get_option("errors") == 0


def test_automask_local_is_the_two_calls_it_replaces(ctx):
    from test_gpu_imager import Case
    img, _, outside = ramp_image(0)
    N = img.shape[0]
    kw = dict(border=1, step=16, half=16, kappa=3.0, nclip=3, min_count=16)
    akw = dict(nsigma=(5, 2.5), min_cells=2, grow=1, absolute=True)
    start = np.zeros((N, N), dtype=np.uint8)
    start[N // 2 - 5:N // 2 + 6, N // 2 - 5:N // 2 + 6] = 1  # a mask over the source: its cells stay out of the noise estimate
    _, _, snr, _, nst = ctx.noise_map(to_dev(img), to_dev(start), exclude=True, mode="snr", maps=False, **kw)
    m2, ast = ctx.automask(snr, to_dev(start), border=1, absolute=True, thr=(5, 2.5), nsigma=(0, 0), min_cells=2, grow=1)
    want = [host(t) for t in (m2, ast, snr, nst)]
    compare([host(snr), host(nst)], [x for x in ref.noise_map(img, start, exclude=True, mode="snr", **kw)[2:5:2]], "snr")
    c = Case(ctx, "simple", 0.1, 1920, 600, 7)  # an imager of N = 192
    assert c.N == N
    for who, a, m in ((ctx, to_dev(img), to_dev(start)), (c.im, to_dev(img), to_dev(start)), (ctx, img, start.copy())):
        got = who.automask_local(a, m, **kw, **akw)
        assert got[0] is m
        for g, w in zip(got, want):
            g = host(g) if hasattr(g, "cpu") else g
            assert g.dtype == w.dtype and same(g.astype(np.float64), w.astype(np.float64))
    c.im.close()
    # without a mask every cell takes part; at one level, components of one cell and no growing the mask IS the cells above
    # 4 local sigma, and the restatement says how many of them are noise: the same count, not a tolerance
    mask, ast, snr, nst = ctx.automask_local(to_dev(img), None, step=16, half=16, nclip=3, nsigma=(4, 4))
    w_snr = ref.noise_map(img, None, step=16, half=16, nclip=3, mode="snr")[2]
    assert same(host(snr), w_snr)
    assert np.array_equal(host(mask) != 0, w_snr > 4.0)
    n_local = int(np.count_nonzero((host(mask) != 0) & outside))
    g = noise_ref.image_stats(img)
    n_global = int(np.count_nonzero((img > g[1] + 4.0 * g[3]) & outside))
    assert n_local == int(np.count_nonzero((w_snr > 4.0) & outside)) == 4 and n_global == 57


def test_refusals(ctx):
    """every argument the header refuses, in the host and the _dev form: the code, and nothing touched"""
    import torch
    import gridhip
    EINVAL, EUNSUPPORTED = gridhip._lib.EINVAL, gridhip._lib.EUNSUPPORTED
    N = 8
    f64 = dict(dtype=torch.float64, device="cuda:0")
    img = torch.full((N * N,), 1.5, **f64)
    mask = torch.full((N * N,), 5, dtype=torch.uint8, device="cuda:0")
    outs = {k: torch.full((n,), 7.0, **f64) for k, n in (("nodes", 4), ("background", N * N), ("rms", N * N), ("out", N * N),
                                                         ("stats", 8))}
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    order = ("N", "image", "mask", "exclude", "border", "step", "half", "kappa", "nclip", "min_count", "mode", "nodes",
             "background", "rms", "out", "stats")
    base = dict(N=N, image=p(img), mask=p(mask), exclude=0, border=0, step=16, half=4, kappa=3.0, nclip=3, min_count=4, mode=2,
                **{k: p(v) for k, v in outs.items()})
    einval = [dict(N=0), dict(border=-1), dict(border=4), dict(step=0), dict(half=0), dict(kappa=0.0), dict(kappa=-1.0),
              dict(kappa=float("nan")), dict(kappa=float("inf")), dict(nclip=-1), dict(nclip=9), dict(min_count=0),
              dict(exclude=2), dict(exclude=-1), dict(mode=3), dict(mode=-1), dict(image=None), dict(stats=None),
              dict(out=None), dict(out=None, mode=1),
              # overlaps: only out may be the image, and then exactly
              dict(nodes=p(img)), dict(background=p(img)), dict(rms=p(mask)), dict(out=p(img, 8)),
              dict(stats=p(img, 8 * N * N - 8)),
              dict(out=p(outs["background"])), dict(rms=p(outs["background"], 8 * N * N - 8)), dict(stats=p(outs["nodes"], 24)),
              dict(nodes=p(outs["stats"])), dict(out=p(mask)),
              dict(half=65, step=0)]  # EINVAL comes first
    lib, h = ctx._lib, ctx._h
    ctx._use_torch_stream()
    for change, code in [(x, EINVAL) for x in einval] + [(dict(half=65), EUNSUPPORTED), (dict(N=1048561), EUNSUPPORTED)]:
        args = [dict(base, **change)[k] for k in order]
        assert lib.gridhip_noise_map_dev(h, *args) == code, change
        assert lib.gridhip_noise_map(h, *args) == code, change
    assert lib.gridhip_noise_map_dev(None, *[base[k] for k in order]) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(img == 1.5) and torch.all(mask == 5) and all(torch.all(v == 7.0) for v in outs.values())
    # what is allowed: out == image, and the limits themselves
    assert lib.gridhip_noise_map_dev(h, *[dict(base, out=p(img), half=64, nclip=8)[k] for k in order]) == 0
    torch.cuda.synchronize()
    # the Python layer's own rules
    with pytest.raises(ValueError):
        ctx.noise_map(np.zeros((4, 5)))
    with pytest.raises(ValueError):
        ctx.noise_map(np.zeros((4, 4)), mode="divide")
    with pytest.raises(gridhip.GridHipError):
        ctx.noise_map(np.zeros((4, 4)), border=2)
