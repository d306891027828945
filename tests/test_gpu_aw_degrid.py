"""GPU checks of the aw degridder (degrid4 / gridhip_awdegrid) and of aw plans (gridhip_aw_plan): parity with a numpy
restatement of the gather, the adjoint identity against convgrid4, host and device forms, the tap-reusing and the
general tile kernel, and plans that keep their kernels, records and tables between passes.  The reference has no
degrid: parity is with the definition in include/gridhip.h (unpinned, like degrid2's)."""
import ctypes as C

import numpy as np
import pytest

from oracle import gridref_np as P

pytestmark = pytest.mark.gpu
TOL = 1e-10
BIG = (1 << 20) + 3000  # crosses the 2^20-visibility batch of the aw kernel table


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def awdegrid_np(wk, ak, G, u, v, wb, a1, a2):
    """vis_out[k] = sum_ij conj(aw_kernel_fn2(yf, xf, wk[wb], ak[a1], ak[a2]))[i, j] * G[y0 + i, x0 + j], taps outside
    the grid 0, out-of-range indices 0 (include/gridhip.h)."""
    W, Q, _, S, _ = wk.shape
    A = ak.shape[0]
    H, Wd = G.shape
    x, xf, y, yf = P.frac_coords((H, Wd), Q, u, v)
    out = np.zeros(len(u), dtype=np.complex128)
    kern = {}
    for k in range(len(u)):
        if not (0 <= wb[k] < W and 0 <= a1[k] < A and 0 <= a2[k] < A):
            continue
        key = (int(wb[k]), int(yf[k]), int(xf[k]), int(a1[k]), int(a2[k]))
        if key not in kern:
            kern[key] = np.conj(P.aw_kernel_fn2(key[1], key[2], wk[key[0]], ak[key[3]], ak[key[4]]))
        ys, xs = np.arange(S) + (y[k] - S // 2), np.arange(S) + (x[k] - S // 2)
        my, mx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < Wd)
        out[k] = (kern[key][np.ix_(my, mx)] * G[np.ix_(ys[my], xs[mx])]).sum()
    return out


def case(seed, H, Wd, W, Q, S, A, n):
    rng = np.random.default_rng(seed)
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    # footprints over every edge and corner of the grid
    edge = np.array([-0.5, 0.4999, 0.0])
    eu, ev = np.meshgrid(edge, edge)
    u[:9], v[:9] = eu.ravel(), ev.ravel()
    wb, a1, a2 = rng.integers(0, W, n), rng.integers(0, A, n), rng.integers(0, A, n)
    G = rng.normal(size=(H, Wd)) + 1j * rng.normal(size=(H, Wd))
    return wk, ak, u, v, wb, a1, a2, G


@pytest.mark.parametrize("H,Wd,W,Q,S,A,n,path", [
    (64, 80, 3, 2, 15, 6, 1500, 1), (72, 56, 2, 4, 7, 12, 1500, 1), (50, 70, 4, 1, 9, 3, 1200, 1),
    (64, 60, 2, 2, 16, 4, 800, 1), (40, 52, 2, 2, 5, 4, 1500, 1), (64, 72, 2, 2, 4, 5, 1000, 3),
    (90, 70, 2, 2, 19, 3, 500, 3)])
def test_degrid4_matches_restatement(ctx, H, Wd, W, Q, S, A, n, path):
    wk, ak, u, v, wb, a1, a2, G = case(H * 100 + S, H, Wd, W, Q, S, A, n)
    # out-of-range w-bins and antennas: exact zeros, counted
    bad = [(20, "wb", W), (31, "wb", -1), (42, "a1", -1), (53, "a1", A), (64, "a2", A), (75, "a2", -3)]
    arrs = {"wb": wb, "a1": a1, "a2": a2}
    for k, name, val in bad:
        arrs[name][k] = val
    ref = awdegrid_np(wk, ak, G, u, v, wb, a1, a2)
    try:
        for cache in (1, 0):
            ctx.set_option("aw_cache", cache)
            got = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2))
            assert ctx.get_option("last_path") == path
            assert rel(got, ref) < TOL, cache
            assert all(got[k] == 0 for k, _, _ in bad)
            assert ctx.last_dropped() == len(bad) and ctx.get_option("errors") == 0
    finally:
        ctx.set_option("aw_cache", 1)


def test_degrid4_overwrites_and_empty(ctx):
    wk, ak, u, v, wb, a1, a2, G = case(7, 48, 48, 2, 2, 9, 3, 300)
    out = np.full(300, 7 + 7j)
    got = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2), out=out)
    assert got is out and rel(out, awdegrid_np(wk, ak, G, u, v, wb, a1, a2)) < TOL
    e = np.zeros(0)
    assert ctx.degrid4(wk, ak, G, (e, e, None), (e.astype(np.int64),) * 3).shape == (0,)


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_host_dev_and_sorted_general_agree(ctx):
    import torch
    wk, ak, u, v, wb, a1, a2, G = case(11, 256, 192, 4, 4, 15, 16, 20000)
    host = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2))
    assert ctx.get_option("last_path") == 1
    dev = ctx.degrid4(t(wk), t(ak), t(G), (t(u), t(v), None), (t(wb), t(a1), t(a2)))
    torch.cuda.synchronize()
    assert rel(dev.cpu().numpy(), host) <= 1e-12
    try:
        ctx.set_option("sort", 2)
        gen = ctx.degrid4(wk, ak, G, (u, v, None), (wb, a1, a2))
        assert ctx.get_option("last_path") == 3
    finally:
        ctx.set_option("sort", 0)
    assert rel(gen, host) <= 1e-12


def adjoint_err(ctx, wk, ak, u, v, wb, a1, a2, vis, g):
    import torch
    Gs = ctx.convgrid4(wk, ak, torch.zeros_like(g), (u, v, None), (wb, a1, a2), vis)
    d = ctx.degrid4(wk.conj().resolve_conj(), ak.conj().resolve_conj(), g, (u, v, None), (wb, a1, a2))
    lhs = torch.vdot(g.flatten(), Gs.flatten()).item()
    rhs = torch.vdot(d, vis).item()
    return abs(lhs - rhs) / abs(lhs)


def big_stream(seed, n, N=1024, W=8, Q=4, S=15, A=32):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    cplx = lambda *s: torch.complex(torch.randn(*s, generator=g, device="cuda:0", dtype=torch.float64),
                                    torch.randn(*s, generator=g, device="cuda:0", dtype=torch.float64))
    wk, ak = cplx(W, Q, Q, S, S), cplx(A, S, S)
    u = torch.rand(n, generator=g, device="cuda:0", dtype=torch.float64) - 0.5
    v = torch.rand(n, generator=g, device="cuda:0", dtype=torch.float64) - 0.5
    ints = lambda hi: torch.randint(0, hi, (n,), generator=g, device="cuda:0")
    return wk, ak, u, v, ints(W), ints(A), ints(A), cplx(n), cplx(N, N)


@pytest.mark.parametrize("n", [20000, BIG])
def test_adjointness(ctx, n):
    err = adjoint_err(ctx, *big_stream(n, n))
    assert err < 1e-11 and ctx.get_option("errors") == 0


@pytest.mark.parametrize("n", [5000, BIG])
def test_plan_matches_calls(ctx, n):
    import torch
    wk, ak, u, v, wb, a1, a2, vis, g = big_stream(3 + n, n)
    G0 = ctx.convgrid4(wk, ak, torch.zeros_like(g), (u, v, None), (wb, a1, a2), vis)
    d0 = ctx.degrid4(wk, ak, g, (u, v, None), (wb, a1, a2))
    plan = ctx.aw_plan(g.shape, wk, ak, (u, v, None), (wb, a1, a2))
    assert ctx.get_option("aw_tables_built") == (2 if n == BIG else 1)
    st = ctx.aw_stats(15)
    assert st["vis_keyed"] == n and ctx.last_dropped() == 0
    # the plan keeps its kernels and records: the caller's arrays may change
    for x in (wk, ak, u, v):
        x.fill_(0.25)
    for x in (wb, a1, a2):
        x.fill_(10 ** 6)
    torch.cuda.synchronize()
    for _ in range(2):
        G = plan.grid(torch.zeros_like(g), vis)
        assert ctx.get_option("aw_tables_built") == 0
        d = plan.degrid(g)
        assert ctx.get_option("aw_tables_built") == 0 and ctx.get_option("last_path") == 1
        torch.cuda.synchronize()
        assert (G - G0).abs().max().item() <= 1e-12 * G0.abs().max().item()
        assert (d - d0).abs().max().item() <= 1e-12 * d0.abs().max().item()
    # grid accumulates
    G2 = plan.grid(G.clone(), vis)
    assert (G2 - 2 * G0).abs().max().item() <= 1e-12 * G0.abs().max().item()
    assert ctx.get_option("errors") == 0
    plan.close()


def test_alternating_plans_and_dropped(ctx):
    """two plans over different baselines on one context: nothing of one leaks into the other; a plan whose stream has
    out-of-range indices predicts exactly 0 there (its degrid clears vis_out) and reports them as dropped"""
    import torch
    sa = big_stream(21, 6000, N=256, W=3, Q=2, S=9, A=5)
    sb = big_stream(22, 4000, N=256, W=3, Q=2, S=9, A=5)
    sb[4][::97] = 3  # wbin out of range
    nbad = len(range(0, 4000, 97))
    ref = []
    for wk, ak, u, v, wb, a1, a2, vis, g in (sa, sb):
        ref.append((ctx.convgrid4(wk, ak, torch.zeros_like(g), (u, v, None), (wb, a1, a2), vis),
                    ctx.degrid4(wk, ak, g, (u, v, None), (wb, a1, a2))))
    pa = ctx.aw_plan(sa[8].shape, *sa[:2], (sa[2], sa[3], None), sa[4:7])
    assert ctx.last_dropped() == 0
    pb = ctx.aw_plan(sb[8].shape, *sb[:2], (sb[2], sb[3], None), sb[4:7])
    assert ctx.last_dropped() == nbad
    for _ in range(2):
        for pl, s, (G0, d0) in ((pa, sa, ref[0]), (pb, sb, ref[1])):
            out = torch.full_like(d0, 5 + 5j)
            d = pl.degrid(s[8], out=out)
            G = pl.grid(torch.zeros_like(s[8]), s[7])
            torch.cuda.synchronize()
            assert (d - d0).abs().max().item() <= 1e-12 * d0.abs().max().item()
            assert (G - G0).abs().max().item() <= 1e-12 * G0.abs().max().item()
    assert (d[::97] == 0).all()
    pa.close()
    pb.close()


def test_plan_edge_cases(ctx):
    import torch
    from gridhip import _lib
    lib, h = ctx._lib, ctx._h
    wk, ak, u, v, wb, a1, a2, vis, g = big_stream(5, 100, N=64, W=2, Q=2, S=7, A=3)
    ctx._use_torch_stream()  # (the raw calls below run on the context's stream: torch's, where the inputs were made)
    p = lambda x: C.c_void_p(x.data_ptr())
    pl = C.c_void_p()
    args = [h, 64, 64, 100, 2, 2, 7, 3, p(wk), p(ak), p(u), p(v), 1, p(wb), p(a1), p(a2)]
    # n = 0: a plan with nothing to do
    a0 = list(args)
    a0[3] = 0
    assert lib.gridhip_aw_plan_create_dev(*a0, C.byref(pl)) == 0 and pl.value
    assert lib.gridhip_aw_plan_grid_dev(pl, None, p(g)) == 0
    assert lib.gridhip_aw_plan_degrid_dev(pl, p(g), None) == 0
    assert lib.gridhip_aw_plan_grid_dev(pl, None, None) == _lib.EINVAL
    assert lib.gridhip_aw_plan_destroy(pl) == 0
    # null pointers
    for i in (8, 9, 10, 13, 15):
        bad = list(args)
        bad[i] = None
        assert lib.gridhip_aw_plan_create_dev(*bad, C.byref(pl)) == _lib.EINVAL
    assert lib.gridhip_aw_plan_create_dev(*args, None) == _lib.EINVAL
    assert lib.gridhip_aw_plan_grid_dev(None, p(vis), p(g)) == _lib.EINVAL
    assert lib.gridhip_aw_plan_degrid_dev(None, p(g), p(vis)) == _lib.EINVAL
    assert lib.gridhip_aw_plan_destroy(None) == 0
    assert lib.gridhip_aw_plan_create_dev(*args, C.byref(pl)) == 0
    assert lib.gridhip_aw_plan_grid_dev(pl, None, p(g)) == _lib.EINVAL
    assert lib.gridhip_aw_plan_degrid_dev(pl, None, p(vis)) == _lib.EINVAL
    assert lib.gridhip_aw_plan_degrid_dev(pl, p(g), None) == _lib.EINVAL
    assert lib.gridhip_aw_plan_destroy(pl) == 0
    dv = lambda *a: lib.gridhip_awdegrid_dev(h, 64, 64, *a)
    assert dv(p(g), 100, 2, 2, 7, 3, p(wk), p(ak), p(u), p(v), 1, p(wb), p(a1), p(a2), None) == _lib.EINVAL
    assert dv(None, 100, 2, 2, 7, 3, p(wk), p(ak), p(u), p(v), 1, p(wb), p(a1), p(a2), p(vis)) == _lib.EINVAL
    # S > 63
    big = torch.zeros(64 * 64 * 4, dtype=torch.complex128, device="cuda:0")
    a64 = list(args)
    a64[6], a64[8], a64[9] = 64, p(big), p(big)
    assert lib.gridhip_aw_plan_create_dev(*a64, C.byref(pl)) == _lib.EUNSUPPORTED
    assert dv(p(g), 100, 2, 2, 64, 3, p(big), p(big), p(u), p(v), 1, p(wb), p(a1), p(a2), p(vis)) == _lib.EUNSUPPORTED
    # a closed plan of either kind refuses a pass before it reaches the library
    gcf = torch.zeros((2, 2, 2, 7, 7), dtype=torch.complex128, device="cuda:0")
    aw = ctx.aw_plan(g.shape, wk, ak, (u, v, None), (wb, a1, a2))
    w2 = ctx.plan(g.shape, gcf.shape, (u, v, None), wb)
    aw.grid(g, vis), w2.grid(gcf, g, vis)
    aw.close(), w2.close()
    aw.close(), w2.close()  # (closing twice is harmless)
    for call in (lambda: aw.grid(g, vis), lambda: aw.degrid(g), lambda: w2.grid(gcf, g, vis), lambda: w2.degrid(gcf, g)):
        with pytest.raises(AssertionError, match="plan is closed"):
            call()
