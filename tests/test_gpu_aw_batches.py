"""The aw batch loop (csrc/awgrid.hip: aw_batches, gridhip_aw_plan_create_dev, and the entry points above them) at batch
sizes an oracle can follow (option "aw_batch"): every batch after the first against oracle.awgrid(direct=True) and the
numpy restatement of the gather, not against another run of the same loop.  The fixtures are tests/aw_batch_cases.py's,
whose properties tests/test_aw_batches_host.py shows on the CPU: structure at the cuts (exact multiple, a last batch
of one, one visibility per batch, a run of equal keys across a cut, a batch of dropped visibilities only, a batch whose
pair is older than itself) and hash keys whose probe goes round the end of the 1024-slot table.

Tolerances: 1e-10 of the reference's largest magnitude against the oracle (tests/test_gpu_aw.py, test_gpu_aw_degrid.py,
test_gpu_imager.py, test_gpu_aw_imaging.py: theirs), 1e-12 between a split and an unsplit evaluation of the same sums on
the GPU (test_gpu_aw_degrid.py's figure for two GPU evaluations).  The counters are exact; last_dropped() counts the
indices out of range, not the NaN coordinates (aw_batch_cases.py says why).  47 cases, 7 s on an MI355X."""
import functools

import numpy as np
import pytest

import aw_batch_cases as E
from oracle import gridref_np as P

pytestmark = pytest.mark.gpu
TOL = 1e-10
SAME = 1e-12
FILL = 5 + 5j


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def t(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def host(x):
    return x.cpu().numpy()


class options:
    """context options for a block; all of them back at their defaults afterwards"""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        self.ctx.set_option("aw_batch", 0)
        self.ctx.set_option("aw_cache", 1)
        self.ctx.set_option("sort", 0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(start grid, gridded reference, grid to gather from, gathered reference, kept, figures) of a fixture, once"""
    from oracle import gridref_c as oracle
    from test_gpu_aw_degrid import awdegrid_np
    c = E.by_name(name)
    keep = E.kept(c)
    rng = np.random.default_rng(len(name) + c.N)
    start = rng.normal(size=(c.N, c.N)) + 1j * rng.normal(size=(c.N, c.N))
    gref = oracle.awgrid(c.wk, c.ak, start.copy(), c.u[keep], c.v[keep], c.wb[keep], c.a1[keep], c.a2[keep], c.vis[keep],
                         direct=True)
    G = rng.normal(size=(c.N, c.N)) + 1j * rng.normal(size=(c.N, c.N))
    ru, rv, rwb = E.for_the_restatement(c)
    dref = awdegrid_np(c.wk, c.ak, G, ru, rv, rwb, c.a1, c.a2)
    assert (dref[~keep] == 0).all() and (dref[keep] != 0).all()
    for a in (start, gref, G, dref):
        a.setflags(write=False)
    return start, gref, G, dref, keep, E.figures(c, oracle.frac_coord)


def check_counters(ctx, c, cache, figs, tables):
    per, total, dropped, _ = figs
    n = len(c.u)
    st = ctx.aw_stats(c.S)
    assert st["vis_keyed"] == n
    assert st["kernels_built"] == (total if cache else n), (st, total)
    assert ctx.last_dropped() == dropped
    assert ctx.get_option("aw_tables_built") == tables
    assert ctx.get_option("errors") == 0


def check_gather(got, dref, keep):
    assert rel(got, dref) < TOL, rel(got, dref)
    assert (got[~keep] == 0).all()       # every dropped visibility exactly 0, in every batch
    assert not (got == FILL).any()       # no element keeps the fill


@pytest.mark.parametrize("sort", [0, 2])
@pytest.mark.parametrize("cache", [1, 0])
@pytest.mark.parametrize("name", [c.name for c in E.all_cases()])
def test_calls_and_plans_against_the_oracle(ctx, name, cache, sort):
    """convgrid4 onto a non-zero grid, degrid4 into a filled output, and an aw plan's grid and degrid (twice each, the
    caller's arrays overwritten), each split into batches of B against the oracle; the counters; the split call against
    the unsplit one."""
    import torch
    c = E.by_name(name)
    start, gref, G, dref, keep, figs = reference(name)
    n, nb = len(c.u), -(-len(c.u) // c.B)
    p, idx = (c.u, c.v, None), (c.wb, c.a1, c.a2)
    with options(ctx, aw_cache=cache, sort=sort):
        whole_g = ctx.convgrid4(c.wk, c.ak, start.copy(), p, idx, c.vis)
        assert ctx.get_option("aw_tables_built") == 1
        whole_d = ctx.degrid4(c.wk, c.ak, G, p, idx, out=np.full(n, FILL))
        ctx.set_option("aw_batch", c.B)
        # gridding
        got = ctx.convgrid4(c.wk, c.ak, start.copy(), p, idx, c.vis)
        check_counters(ctx, c, cache, figs, nb)
        print(name, cache, sort, "grid", rel(got, gref), "split/unsplit", rel(got, whole_g))
        assert rel(got, gref) < TOL and rel(whole_g, gref) < TOL
        assert rel(got, whole_g) < SAME
        # degridding
        out = np.full(n, FILL)
        d = ctx.degrid4(c.wk, c.ak, G, p, idx, out=out)
        assert d is out and (sort != 2 or ctx.get_option("last_path") == 3)  # (the general tile kernel where asked for)
        check_counters(ctx, c, cache, figs, nb)
        print(name, cache, sort, "degrid", rel(d, dref), "split/unsplit", rel(d, whole_d))
        check_gather(d, dref, keep)
        check_gather(whole_d, dref, keep)
        assert rel(d, whole_d) < SAME
        # a plan made with the batch size; it records its batches, whatever the option says later
        dev = [t(x) for x in (c.wk, c.ak, c.u, c.v, c.wb, c.a1, c.a2)]
        plan = ctx.aw_plan((c.N, c.N), dev[0], dev[1], (dev[2], dev[3], None), tuple(dev[4:7]))
        check_counters(ctx, c, cache, figs, nb)
        ctx.set_option("aw_batch", 0)
        for x in dev[:4]:
            x.fill_(0.25)
        for x in dev[4:]:
            x.fill_(10 ** 6)
        dvis, dG = t(c.vis), t(G)
        torch.cuda.synchronize()
        for _ in range(2):
            pg = plan.grid(t(start), dvis)
            assert ctx.get_option("aw_tables_built") == 0
            pd = plan.degrid(dG, out=torch.full((n,), FILL, dtype=torch.complex128, device="cuda:0"))
            assert ctx.get_option("aw_tables_built") == 0
            torch.cuda.synchronize()
            assert rel(host(pg), gref) < TOL
            check_gather(host(pd), dref, keep)
        assert ctx.get_option("errors") == 0
        plan.close()


def test_do_imaging_aw_in_batches(ctx, oracle):
    """two passes (image and PSF) over one batch loop: against test_do_imaging_aw_matches_oracle_at_driver_size's chain"""
    from test_gpu_aw_imaging import oracle_imgfn
    c = E.by_name("plus-one")
    theta = 0.008
    lam, wv, (u, v, w) = E.imaging_form(c, theta)
    uvw = np.stack([u, v, w], axis=1)
    vis, a1, a2 = np.array(c.vis), np.array(c.a1), np.array(c.a2)
    ri, rp, rm = P.do_imaging(theta, lam, u, v, w, vis, oracle_imgfn(oracle, c.wk, wv, c.ak, a1, a2))
    for cache in (1, 0):
        with options(ctx, aw_cache=cache, aw_batch=c.B):
            img, psf, pmax = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", c.wk, wv, c.ak))
            assert ctx.get_option("aw_tables_built") == -(-len(u) // c.B)  # one table per batch for both passes
            assert ctx.aw_stats(c.S)["vis_keyed"] == len(u) and ctx.last_dropped() == 0
            assert ctx.get_option("errors") == 0
        print(cache, rel(img, ri), rel(psf, rp), abs(pmax - rm) / abs(rm))
        assert img.shape == (c.N, c.N)
        assert rel(img, ri) < 1e-10
        assert rel(psf, rp) < 1e-10
        assert abs(pmax - rm) <= 1e-10 * abs(rm)
        with options(ctx, aw_cache=cache):
            img0, psf0, pmax0 = ctx.do_imaging(theta, lam, uvw, a1, a2, None, None, vis, ("aw", c.wk, wv, c.ak))
        assert rel(img, img0) < SAME and rel(psf, psf0) < SAME and abs(pmax - pmax0) <= SAME * abs(pmax0)


def test_imager_in_batches(ctx):
    """an aw imager whose two plans hold several batches: one cycle and one predict against test_gpu_imager.py's numpy
    side"""
    import torch
    import test_gpu_imager as I
    c = E.by_name("straddle")
    theta = 0.008
    lam, wv, uvw = E.imaging_form(c, theta)
    rng = np.random.default_rng(9)
    im = I.Case.__new__(I.Case)
    im.ctx, im.kind, im.theta, im.lam, im.N = ctx, "aw", theta, lam, c.N
    im.uvw, im.vis, im.model, im.kv = uvw, np.array(c.vis), rng.normal(size=(c.N, c.N)), None
    im.aw = (np.array(c.wk), wv, np.array(c.ak), np.array(c.a1), np.array(c.a2))
    img_ref, _, psf_ref, pmax_ref, pred_ref, res_ref = I.numpy_side("aw", theta, lam, im.uvw, im.vis, im.model, None, im.aw)
    with options(ctx, aw_batch=c.B):
        im.bind()
        assert ctx.get_option("aw_tables_built") == 2 * -(-len(c.u) // c.B)  # the batches of two streams
        assert ctx.get_option("errors") == 0
    vis_res = torch.empty_like(im.dvis)
    img = im.cycle(im.dvis, im.dmodel, vis_res=vis_res)
    figs = {"image": rel(host(img), img_ref), "psf": rel(host(im.im.psf), psf_ref),
            "pmax": abs(im.im.pmax - pmax_ref) / abs(pmax_ref), "predict": rel(host(im.im.predict(im.dmodel)), pred_ref),
            "vis_res": rel(host(vis_res), res_ref)}
    print(figs)
    assert np.abs(img_ref).max() > 0 and np.abs(pred_ref).max() > 0 and pmax_ref > 0
    assert max(figs.values()) < 1e-10, figs
    im.im.close()


def test_a_negative_batch_is_refused(ctx):
    """by convgrid4, degrid4 and aw_plan, with EINVAL, before anything is touched"""
    import ctypes as C
    from gridhip import _lib
    c = E.by_name("multiple")
    n = len(c.u)
    lib, h = ctx._lib, ctx._h
    wk, ak, u, v, wb, a1, a2, vis = (np.array(x) for x in c[6:14])
    grid, out = np.full((c.N, c.N), FILL), np.full(n, FILL)
    q = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    args = [n, c.W, c.Q, c.S, c.A, q(wk), q(ak), q(u), q(v), 1, q(wb), q(a1), q(a2)]
    dev = [t(x) for x in (wk, ak, u, v, wb, a1, a2)]
    dq = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    pl = C.c_void_p(0x1234)
    try:
        ctx.set_option("aw_batch", -1)
        assert ctx.get_option("aw_batch") == -1
        assert lib.gridhip_awgrid(h, c.N, c.N, q(grid), *args, q(vis)) == _lib.EINVAL
        assert "aw_batch" in ctx._error(_lib.EINVAL)
        assert lib.gridhip_awdegrid(h, c.N, c.N, q(grid), *args, q(out)) == _lib.EINVAL
        assert lib.gridhip_aw_plan_create_dev(h, c.N, c.N, n, c.W, c.Q, c.S, c.A, dq(dev[0]), dq(dev[1]), dq(dev[2]),
                                              dq(dev[3]), 1, dq(dev[4]), dq(dev[5]), dq(dev[6]), C.byref(pl)) == _lib.EINVAL
        assert not pl.value
        with pytest.raises(Exception, match="aw_batch"):
            ctx.convgrid4(wk, ak, grid, (u, v, None), (wb, a1, a2), vis)
        with pytest.raises(Exception, match="aw_batch"):
            ctx.degrid4(wk, ak, grid, (u, v, None), (wb, a1, a2), out=out)
        with pytest.raises(Exception, match="aw_batch"):
            ctx.aw_plan((c.N, c.N), dev[0], dev[1], (dev[2], dev[3], None), tuple(dev[4:7]))
    finally:
        ctx.set_option("aw_batch", 0)
    assert (grid == FILL).all() and (out == FILL).all()
    # the context is as usable as before
    start, gref, _, _, _, _ = reference("multiple")
    assert rel(ctx.convgrid4(wk, ak, start.copy(), (u, v, None), (wb, a1, a2), vis), gref) < TOL


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_awgrid_batched(ctx, oracle, seed):
    """test_gpu_fuzz.py's test_fuzz_awgrid draws (its own seeds), and a batch size from {1, 7, n // 3 + 1, n - 1, n,
    n + 1}: gridding and degridding against the oracle"""
    from test_gpu_aw_degrid import awdegrid_np
    rng = np.random.default_rng(9000 + seed)
    S = int(rng.choice([3, 5, 7, 9, 11, 13, 15, 8, 12, 16, 19]))
    N = int(rng.integers(2 * S + 4, 260))
    W, Q, A = int(rng.choice([1, 2, 5])), int(rng.choice([1, 2, 4])), int(rng.choice([2, 3, 9]))
    nb = int(rng.choice([1, 5, 60, 400]))
    dumps = int(rng.choice([1, 3, 8]))
    n = nb * dumps
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    u0, v0 = rng.uniform(-0.55, 0.55, nb), rng.uniform(-0.55, 0.55, nb)
    drift = float(rng.choice([0.0, 0.02, 0.3])) / N
    d = np.arange(dumps)
    u = (u0[:, None] + d[None, :] * drift).ravel()
    v = (v0[:, None] - d[None, :] * drift).ravel()
    rep = lambda a: np.repeat(a, dumps)  # noqa: E731
    wb, a1, a2 = rep(rng.integers(0, W, nb)), rep(rng.integers(0, A, nb)), rep(rng.integers(0, A, nb))
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    if n > 4:
        wb[1], a2[3] = W + 2, -5
    keep = (wb >= 0) & (wb < W) & (a2 >= 0)
    start = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N))
    ref = oracle.awgrid(wk, ak, start.copy(), u[keep], v[keep], wb[keep], a1[keep], a2[keep], vis[keep], direct=True)
    dref = awdegrid_np(wk, ak, start, u, v, wb, a1, a2)
    cache = int(rng.integers(0, 2))
    sort = int(rng.choice([0, 2]))
    B = int(rng.choice([1, 7, n // 3 + 1, n - 1, n, n + 1])) if n > 1 else 1
    with options(ctx, aw_cache=cache, sort=sort, aw_batch=B):
        got = ctx.convgrid4(wk, ak, start.copy(), (u, v, None), (wb, a1, a2), vis)
        st, tables = ctx.aw_stats(S), ctx.get_option("aw_tables_built")
        errors = ctx.get_option("errors")
        dgot = ctx.degrid4(wk, ak, start, (u, v, None), (wb, a1, a2), out=np.full(n, FILL))
        errors += ctx.get_option("errors")
    what = (S, N, W, Q, A, nb, dumps, cache, sort, B)
    print(what, rel(got, ref), rel(dgot, dref))
    assert errors == 0
    assert rel(got, ref) < TOL, what
    assert rel(dgot, dref) < TOL and (dgot[~keep] == 0).all() and not (dgot == FILL).any(), what
    assert tables == -(-n // min(B, n)) and st["vis_keyed"] == n, what
    assert st["kernels_built"] == n if not cache else st["kernels_built"] <= max(int(keep.sum()), 1), what
