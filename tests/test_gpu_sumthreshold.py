"""Time-frequency flagging on the device (gridhip_sumthreshold[_dev]) against the numpy restatement
tests/sumthreshold_ref.py.  Every comparison with the restatement is bit for bit - weights, codes, baseline_stats (NaN in
the same places), stats: every output is an order statistic, a count, an integer sum or a fixed tree of rounded additions,
so there is no tolerance to state.  The cubes are the smallest at which each path can go wrong: every direction with
M > L and L == M, the stage kernel's tile either side of its edges with interference laid across them, windows whose hit
flags samples of the next tiles, the last valid window, both orders, the statistics' edge cases, the strict threshold, the
device-resident stop test and rows of the SIR kernels either side of a wave and a work-group."""
import ctypes as C

import numpy as np
import pytest

import sumthreshold_ref as R
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

c128, f64, u8 = np.complex128, np.float64, np.uint8
NAN, INF = np.nan, np.inf


def dev(x):
    return None if x is None else to_dev(x)


def canon(x):
    """NaN positions compared as positions: every NaN becomes the one NaN"""
    x = np.array(x, dtype=f64)
    x[np.isnan(x)] = np.nan
    return x


def run(ctx, vis, model=None, weights=None, form="dev", order="btf", **kw):
    """vis [B][T][F] -> (weights, flags, baseline_stats, stats) as numpy arrays shaped [B][T][F], by the device form (torch
    tensors) or the host form, with the cube handed over in `order`"""
    turn = (lambda x: None if x is None else np.ascontiguousarray(np.swapaxes(x, 0, 1))) if order == "tbf" else (lambda x: x)
    args = [turn(np.asarray(vis, dtype=c128)), turn(None if model is None else np.asarray(model, dtype=c128)),
            turn(None if weights is None else np.asarray(weights, dtype=f64))]
    if form == "host":
        out = ctx.sumthreshold(*args, order=order, **kw)
    else:
        out = tuple(host(x) for x in ctx.sumthreshold(*(dev(x) for x in args), order=order, **kw))
    return turn(out[0]), turn(out[1]), out[2], out[3]


def same(what, got, want):
    w, f, b, s = got
    wr, fr, br, sr = want
    print(f"{what}: stats {s}")
    assert f.dtype == u8 and f.shape == fr.shape and np.array_equal(f, fr), \
        f"{what}: codes differ at {np.argwhere(f != fr)[:8].tolist()}: {f[f != fr][:8]} for {fr[f != fr][:8]}"
    assert R.same_bits(w, wr), f"{what}: weights"
    assert R.same_bits(canon(b), canon(br)), f"{what}: baseline_stats {b} != {br}"
    assert R.same_bits(s, sr), f"{what}: stats {s} != {sr}"


def both(ctx, what, vis, model=None, weights=None, forms=("dev", "host"), orders=("btf",), **kw):
    want = R.sumthreshold(vis, model, weights, **kw)
    got = None
    for order in orders:
        for form in forms:
            got = run(ctx, vis, model, weights, form=form, order=order, **kw)
            same(f"{what} [{form}, {order}]", got, want)
    return got, want


def noise(rng, shape, scale=1.0):
    return scale * (rng.normal(size=shape) + 1j * rng.normal(size=shape))


def lift(vis, add):
    """`add` on the amplitudes of vis"""
    amp = np.abs(vis)
    return vis * ((amp + add) / amp)


@pytest.fixture(scope="module")
def tile():
    import gridhip
    return gridhip.sumthreshold_tile()


# ---- smallest cubes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 1, 8), (1, 1, 16), (1, 1, 32), (1, 1, 64), (1, 1, 65),
                                   (1, 2, 1), (1, 4, 1), (1, 8, 1), (1, 16, 1), (1, 32, 1), (1, 64, 1), (1, 63, 1), (2, 3, 5)])
def test_smallest_cubes(ctx, shape):
    """a row of length L == M for each k (and one either side of 64): the one window j = 0 is the last valid one, and every
    longer window does nothing; the last quarter of a row is lifted, so that windows of several lengths hit"""
    rng = np.random.default_rng(sum(shape))
    vis = noise(rng, shape)
    L = max(shape[1:])
    add = np.zeros(shape)
    add.reshape(shape[0], -1)[:, L - L // 4:] = 3.0
    vis = lift(vis, add)
    (w, f, b, s), _ = both(ctx, f"{shape}", vis, orders=("btf", "tbf"), min_count=1, niter=2)
    (w, f, b, s), _ = both(ctx, f"{shape}, low levels", vis, forms=("dev",), levels=[3.0, 2.0, 1.5, 1.2, 1.0, 0.8, 0.6],
                           min_count=1, niter=4)
    if L >= 8:
        assert s[2] > 0


# ---- tile edges ------------------------------------------------------------------------------------------------------------
def edge_cube(rng, T, F, tt, tf):
    """two baselines of noise; on baseline 0 a burst of four time steps across the first tile boundary in time and a line in
    the channel that ends the first tile in frequency; on baseline 1 a faint line that only the long windows find"""
    vis = noise(rng, (2, T, F))
    add = np.zeros((2, T, F))
    t0 = min(tt, T) - 2
    add[0, max(t0, 0):t0 + 4, :] += 1.5
    add[0, :, min(tf, F) - 1] += 1.0
    add[1, :, min(tf, F - 1)] += 0.7
    return lift(vis, add)


def test_tile_edges(ctx, tile):
    tt, tf = tile
    rng = np.random.default_rng(31)
    shapes = [(T, tf + 1) for T in (tt - 1, tt, tt + 1, 2 * tt + 1)] + [(tt + 1, F) for F in (tf - 1, tf, 2 * tf + 1)]
    for T, F in shapes:
        vis = edge_cube(rng, T, F, tt, tf)
        (w, f, b, s), _ = both(ctx, f"T = {T}, F = {F}", vis, forms=("dev",), orders=("btf", "tbf"))
        assert s[2] > 0
    both(ctx, "the host form", edge_cube(rng, 2 * tt + 1, 2 * tf + 1, tt, tf), forms=("host",))


def test_a_long_window_reaches_into_the_next_two_tiles(ctx, tile):
    """One row of 3 tiles + 5 along frequency (and the same along time): a faint plateau of 64 samples that starts two
    samples before the first tile ends, so the hit window's samples lie in three tiles; only the long windows see it.  And
    a plateau that ends with the row: the hit is in the last valid window j = L - M."""
    tt, tf = tile
    rng = np.random.default_rng(32)
    for axis, tl in ((2, tf), (1, tt)):
        L = 3 * tl + 5
        shape = [2, 3, 3]
        shape[axis] = L
        vis = noise(rng, shape)
        add = np.zeros(shape)
        sl = [0, 1, 1]   # (one line of the cube: the baseline's statistics stay the noise's)
        sl[axis] = slice(tl - 2, tl - 2 + 64)
        add[tuple(sl)] = 1.2
        sl[0], sl[axis] = 1, slice(L - 64, L)
        add[tuple(sl)] = 1.2
        vis = lift(vis, add)
        (w, f, b, s), _ = both(ctx, f"plateaus along axis {axis}", vis, forms=("dev",), orders=("btf", "tbf"), niter=1)
        flagged = f >= 16
        assert flagged[add > 0].mean() > 0.9 and (f[add > 0] % 8 >= 4).any(), "a long window found the plateau"


# ---- statistics edge cases -------------------------------------------------------------------------------------------------
def test_baselines_that_are_not_thresholded_next_to_normal_ones(ctx):
    rng = np.random.default_rng(33)
    B, T, F = 5, 12, 20
    vis = noise(rng, (B, T, F))
    wt = np.ones((B, T, F))
    wt[0] = 0.0                        # all flagged on input: { 0, NaN, NaN, +Inf }
    wt[1].reshape(-1)[5:] = 0.0        # 5 participants: below min_count = 8
    vis[2] = 3 + 4j                    # ties: sigma == 0
    vis[:, 3:5, :] = lift(vis[:, 3:5, :], 3.0)
    (w, f, b, s), _ = both(ctx, "baselines", vis, None, wt, orders=("btf", "tbf"))
    assert (f[0] == 1).all() and b[0, 0] == 0 and np.isnan(b[0, 1:3]).all() and b[0, 3] == INF
    assert b[1, 0] == 5 and np.isfinite(b[1, 1:3]).all() and b[1, 3] == INF and not (f[1] >= 16).any()
    assert b[2].tolist() == [T * F, 5.0, 0.0, INF] and not f[2].any()
    assert (f[3:, 3:5] >= 16).mean() > 0.9 and np.isfinite(b[3:]).all()


def test_non_finite_samples_and_bad_weights_inside_windows(ctx):
    rng = np.random.default_rng(34)
    B, T, F = 2, 40, 70
    vis, mod = noise(rng, (B, T, F)), noise(rng, (B, T, F), 0.1)
    wt = rng.uniform(0.5, 2.0, (B, T, F))
    vis[:, 10:13, :] = lift(vis[:, 10:13, :], 1.5)
    vis[0, :, 33] = lift(vis[0, :, 33], 1.0)
    hole = rng.random((B, T, F))
    vis[hole < 0.01] = NAN
    vis[(hole >= 0.01) & (hole < 0.02)] = INF
    mod[(hole >= 0.02) & (hole < 0.025)] = NAN
    vis[(hole >= 0.025) & (hole < 0.03)] = 1e200
    wt[(hole >= 0.03) & (hole < 0.04)] = 0.0
    wt[(hole >= 0.04) & (hole < 0.05)] = -1.0
    wt[(hole >= 0.05) & (hole < 0.06)] = NAN
    wt[0, 11, :20] = 0.0
    (w, f, b, s), _ = both(ctx, "holes", vis, mod, wt, orders=("btf", "tbf"))
    assert s[3] > 0 and s[6] > 0 and s[2] > 0 and s[4] > 0 and not np.signbit(w).any()
    both(ctx, "no weights", vis, mod, None, forms=("dev",))
    both(ctx, "no model", vis, None, wt, forms=("dev",))


# ---- threshold and ladder ----------------------------------------------------------------------------------------------------
def test_the_threshold_is_strict(ctx):
    a = np.array([0, 0, 0, 1, 1, 1, 2, 2, 0], dtype=f64)
    chi = 2.0 * (1.4826 * 1.0)
    a[-1] = 1.0 + chi
    for shape in ((1, 1, 9), (1, 9, 1)):
        (w, f, b, s), _ = both(ctx, "at chi", a.astype(c128).reshape(shape), levels=[2.0], eta=(0, 0), min_count=1, niter=1)
        assert not f.any() and b[0, 3] == chi
        up = a.copy()
        up[-1] = np.nextafter(a[-1], INF)
        (w, f, b, s), _ = both(ctx, "above chi", up.astype(c128).reshape(shape), levels=[2.0], eta=(0, 0), min_count=1, niter=1)
        assert f.ravel().tolist() == [0] * 8 + [16]
    # a window sum equal to chi * C: 0 0 0 1 1 1 2 2 and a pair whose e sums to 2 chi1 exactly
    row = np.array([0, 0, 0, 1, 1, 1, 2, 2, 0, 0], dtype=f64)
    chi1 = 1.0 * 1.4826
    d = 2.0 ** -52 if np.float64(chi1).view(np.uint64) & 1 else 2.0 ** -51  # (chi1 -+ d have an even last bit: 1 + e is exact)
    row[-2:] = 1.0 + (chi1 - d), 1.0 + (chi1 + d)
    assert (row[-1] - 1.0) + (row[-2] - 1.0) == chi1 * 2.0 and row[-1] - 1.0 == chi1 + d
    (w, f, b, s), _ = both(ctx, "pair at chi", row.astype(c128).reshape(1, 1, 10), levels=[9.0, 1.0], eta=(0, 0), min_count=1, niter=1)
    assert not f.any()


def test_hand_cubes(ctx):
    row = [10, 12, 8, 10, 16, 16, 9, 11]
    (w, f, b, s), _ = both(ctx, "pair", np.array(row, dtype=c128).reshape(1, 1, 8), levels=[5.0, 3.5], eta=(0, 0), min_count=4,
                           niter=3)
    assert f.ravel().tolist() == [0, 0, 0, 0, 17, 17, 0, 0] and s.tolist() == [2, 8, 2, 0, 0, 0, 0, 6]
    a = row[:5] + [1000] + row[5:]
    wt = np.ones(9)
    wt[5] = 0.0
    (w, f, b, s), _ = both(ctx, "flagged inside", np.array(a, dtype=c128).reshape(1, 1, 9), None, wt.reshape(1, 1, 9),
                           levels=[5.0, 3.5], eta=(0, 0), min_count=4, niter=3)
    assert f.ravel().tolist() == [0, 0, 0, 0, 17, 1, 17, 0, 0]


@pytest.mark.parametrize("K,niter", [(1, 2), (7, 0), (7, 1), (7, 4), (3, 4)])
def test_ladder_lengths_and_rounds(ctx, K, niter):
    rng = np.random.default_rng(35)
    vis = noise(rng, (3, 50, 45))
    vis[0, 20:24] = lift(vis[0, 20:24], 1.5)
    vis[1, :, 7] = lift(vis[1, :, 7], 1.0)
    vis[2, 5, 5] = 30.0
    (w, f, b, s), _ = both(ctx, f"K = {K}, niter = {niter}", vis, levels=R.ladder(5.0, 1.5, K), niter=niter)
    assert s[0] <= niter and (niter == 0 or s[2] > 0)
    if niter == 0:
        assert (b[:, 0] == 50 * 45).all() and np.isnan(b[:, 1:3]).all() and (b[:, 3] == INF).all() and s[0] == 0


def test_a_round_that_flags_nothing_stops_the_loop(ctx):
    """one gross spike in noise with high levels: round 0 flags it, round 1 nothing - rounds run is 2 of 4, and the launches
    of the rounds 2 and 3 return at once; the statistics are those round 1 saw"""
    rng = np.random.default_rng(36)
    vis = noise(rng, (2, 30, 40))
    vis[1, 7, 9] = 500.0
    (w, f, b, s), _ = both(ctx, "stop", vis, levels=[12.0, 11.0, 10.0], eta=(0, 0), niter=4)
    assert s[0] == 2 and s[2] == 1 and f[1, 7, 9] == 16 and b[1, 0] == 30 * 40 - 1
    (w, f, b, s), _ = both(ctx, "nothing at all", noise(rng, (2, 30, 40)), levels=[12.0, 11.0], eta=(0, 0), niter=4)
    assert s[0] == 1 and s[2] == 0 and not f.any()


# ---- SIR ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_sir_rows(ctx, L):
    """rows of one and two samples, a wave, a work-group +- 1 and several chunks, along frequency and along time: random
    runs of flags (NaN samples) and of missing cells, an all-flagged and a none-flagged row; eta whose q is odd"""
    rng = np.random.default_rng(L)
    for shape in ((1, 5, L), (1, L, 5)):
        vis = np.ones(shape, dtype=c128)
        wt = np.ones(shape)
        flat_v, flat_w = (x.reshape(5, L) if shape[2] == L else x.reshape(L, 5).T for x in (vis, wt))
        flat_v, flat_w = flat_v.copy(), flat_w.copy()
        for r in (0, 1, 2):
            state = np.cumsum(rng.random(L) < 0.15) % 3   # runs of kept, flagged, kept ...
            flat_v[r, state == 1] = NAN
            flat_w[r, (state == 2) & (rng.random(L) < 0.5)] = 0.0
        flat_v[3, :] = NAN                                 # all flagged; row 4: none
        vis = (flat_v if shape[2] == L else flat_v.T).reshape(shape)
        wt = (flat_w if shape[2] == L else flat_w.T).reshape(shape)
        eta = 314573 / 2.0 ** 20
        assert int(np.rint(eta * 2 ** 20)) % 2 == 1
        for e in ((eta, eta), (eta, 0.0), (0.0, eta), (0.5, 0.99)):
            both(ctx, f"SIR {shape} eta {e}", vis, None, wt, forms=("dev",), eta=e, niter=0)
    both(ctx, "SIR, tbf and host", vis, None, wt, orders=("tbf",), eta=(0.4, 0.4), niter=0)


def test_sir_hand_rows(ctx):
    vis = np.ones((1, 1, 7), dtype=c128)
    vis[0, 0, [1, 2, 4, 5]] = NAN
    for eta, want in ((0.2, [0, 3, 3, 0, 3, 3, 0]), (0.21, [0, 3, 3, 8, 3, 3, 0]), (0.34, [8, 3, 3, 8, 3, 3, 8])):
        (w, f, b, s), _ = both(ctx, f"eta {eta}", vis, eta=(eta, 0.0), niter=0)
        assert f.ravel().tolist() == want
        (w, f, b, s), _ = both(ctx, f"eta {eta} along time", vis.reshape(1, 7, 1), eta=(0.0, eta), niter=0)
        assert f.ravel().tolist() == want


# ---- forms and reruns --------------------------------------------------------------------------------------------------------
def realistic(seed=1):
    return R.interference_cube(seed)


@pytest.fixture(scope="module")
def realistic_want():
    vis, wt, injected = realistic()
    return vis, wt, injected, R.sumthreshold(vis, weights=wt)


def test_the_realistic_cube(ctx, realistic_want):
    vis, wt, injected, want = realistic_want
    got = run(ctx, vis, None, wt)
    same("realistic", got, want)
    same("realistic, tbf", run(ctx, vis, None, wt, order="tbf"), want)
    assert (got[1][injected] >= 16).mean() >= 0.99


def test_in_place_and_two_runs(ctx, realistic_want):
    import torch
    vis, wt, _, want = realistic_want
    dv, dw = dev(vis), dev(wt)
    first = tuple(host(x) for x in ctx.sumthreshold(dv, weights=dw))
    second = tuple(host(x) for x in ctx.sumthreshold(dv, weights=dw))
    same("first run", first, want)
    same("second run", second, want)
    # a repeated call takes no memory
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    out = ctx.sumthreshold(dv, weights=dw, out=dw)
    torch.cuda.synchronize()
    assert out[0] is dw and torch.cuda.mem_get_info()[0] == free
    same("in place", tuple(host(x) for x in out), want)
    assert bool((dv == dev(vis)).all())
    hw = wt.copy()
    out = ctx.sumthreshold(vis, weights=hw, out=hw)
    assert out[0] is hw
    same("host in place", out, want)


def test_a_captured_call_replays_to_the_eager_result(ctx, realistic_want):
    import torch
    vis, wt, _, want = realistic_want
    dv, dw = dev(vis), dev(wt)
    out = torch.empty_like(dw)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds the call's scratch
        ctx.sumthreshold(dv, weights=dw, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        res = ctx.sumthreshold(dv, weights=dw, out=out)
    torch.cuda.synchronize()
    for _ in range(2):
        for x in res:
            x.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        same("replay", [host(x) for x in res], want)
    assert want[3][0] >= 2 and want[3][2] > 0


def test_refusals(ctx):
    """Every rule of the header through the C ABI on device memory, and the outputs as they were given."""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    B, T, F = 2, 3, 4
    n = B * T * F
    full = lambda m, val, dt: torch.full((m,), val, dtype=dt, device="cuda:0")  # noqa: E731
    t = dict(v=full(2 * n, 2 + 1j, torch.complex128), m=full(n, 1 - 1j, torch.complex128), w=full(2 * n, 1.5, torch.float64),
             wo=full(n, 4.0, torch.float64), f=full(n, 9, torch.uint8), bs=full(4 * B, 5.0, torch.float64),
             st=full(8, 6.0, torch.float64))
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    h = ctx._h
    lv = lambda *v: np.array(v, dtype=f64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    keep = [np.array([6.0, 4.0])]
    good = keep[0].ctypes.data_as(C.POINTER(C.c_double))

    def st(B=B, T=T, F=F, order=0, v=p["v"], m=p["m"], w=p["w"], K=2, levels=good, ef=0.2, et=0.2, mc=8, niter=2, wo=p["wo"],
           f=p["f"], bs=p["bs"], s=p["st"]):
        return lib.gridhip_sumthreshold_dev(h, B, T, F, order, v, m, w, K, levels, ef, et, mc, niter, wo, f, bs, s)

    at = lambda key, off: C.c_void_p(t[key].data_ptr() + off)  # noqa: E731
    bad = [st(B=0), st(T=0), st(F=-1), st(order=2), st(order=-1), st(v=None), st(wo=None), st(K=0), st(K=8), st(levels=None),
           st(levels=lv(6.0, 0.0)), st(levels=lv(6.0, -1.0)), st(levels=lv(INF, 1.0)), st(levels=lv(6.0, NAN)),
           st(ef=1.0), st(ef=-0.1), st(ef=NAN), st(et=1.0), st(et=-0.1), st(et=NAN), st(mc=0), st(niter=-1), st(niter=5),
           # an output over an input
           st(wo=p["v"]), st(wo=p["m"]), st(wo=at("w", 8)), st(f=p["v"]), st(f=p["w"]), st(bs=p["m"]), st(bs=p["w"]),
           st(s=at("v", 16 * n - 8)),
           # an output over another output
           st(f=p["wo"]), st(f=at("wo", 8 * n - 1)), st(bs=p["wo"]), st(s=p["wo"]), st(s=p["bs"]), st(s=at("bs", 32 * B - 8)),
           st(bs=p["f"]), st(s=p["f"])]
    torch.cuda.synchronize()
    assert bad == [_lib.EINVAL] * len(bad), bad
    big = [st(B=(1 << 18) + 1, T=1, F=1), st(B=1, T=(1 << 20) + 1, F=1), st(B=1, T=1, F=(1 << 20) + 1), st(B=1 << 12, T=1 << 10, F=1 << 10)]
    assert big == [_lib.EUNSUPPORTED] * len(big), big
    assert st(B=(1 << 18) + 1, K=0) == _lib.EINVAL
    assert lib.gridhip_sumthreshold_dev(None, B, T, F, 0, p["v"], p["m"], p["w"], 2, good, 0.2, 0.2, 8, 2, p["wo"], p["f"],
                                        p["bs"], p["st"]) == _lib.EINVAL
    torch.cuda.synchronize()
    for key, val in (("v", 2 + 1j), ("m", 1 - 1j), ("w", 1.5), ("wo", 4.0), ("f", 9), ("bs", 5.0), ("st", 6.0)):
        assert bool((t[key] == val).all()), key
    # and the valid corners next to them: no model, no weights, no optional output, wt_out == wt_in, an output that ends
    # where an input begins
    assert st(m=None, w=None, f=None, bs=None, s=None) == 0 and st(wo=p["w"], niter=0) == 0
    assert st(wo=at("w", 8 * n), w=p["w"], order=1, ef=0.0, et=0.0) == 0
    ctx.synchronize()


# ---- the clip after the hoist ------------------------------------------------------------------------------------------------
def test_the_clip_is_unchanged(ctx):
    import flag_ref
    import test_gpu_flag as G
    vis, mod, grp, wt = G.stream(np.random.default_rng(5000), 5000, 7)
    want = flag_ref.flag_residuals(vis, mod, group=grp, G=7, weights=wt, nsigma=4.0, niter=3)
    for form in ("dev", "host"):
        G.same(f"clip [{form}]", G.run(ctx, vis, mod, grp, 7, wt, form=form, nsigma=4.0, niter=3), want)
    assert want[3][2] > 0
