"""The binning pre-pass keeps its records when a call's coordinates are unchanged (csrc/bin.hip, "Reuse").

A plain convgrid2 / degrid2 whose key equals the previous call's verifies, in one read-only sweep, that every
pre-record it would derive equals the kept one, and then skips both scatter levels.  Checked here: values-only changes
reuse; any edit of a coordinate that changes a pre-record does not, and the result is the oracle's on the edited stream;
a changed key or an intervening writer of the records never reuses; gridding and degridding share; `bin_reuse` = 1
switches it off; a stream rewritten before every call stops being verified for 4 calls after a failure; a replay of a
graph captured earlier, which the library's host side never sees, is an intervening writer like any other.

Parity is against oracle.gridref_c.convgrid2 at the tolerance of tests/test_gpu_parity.py (1e-10 relative; fp64 atomics
reorder sums).  Shapes: 2^18 visibilities forced onto the two-level path (prepass = 2, sort = 1), a 512^2 grid, 8
planes, Q = 4: about 1100 bins against 256 work-groups; every case at supports 7, 15 and 17 (17: the kernel in parts,
the verify sweep's one-visibility form).  The oracle result of an edited stream is the base result minus
the edited visibility's old contribution plus its new one (one-visibility oracle calls).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10
N, W, Q, NVIS = 512, 8, 4, 1 << 18


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Base:
    """One seeded stream per support, its kernel table and the oracle's grid of it (computed once, never changed)."""

    def __init__(self, oracle, S):
        rng = np.random.default_rng(4000 + S)
        self.S = S
        self.gcf = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
        self.u = rng.uniform(-0.45, 0.45, NVIS)
        self.v = rng.uniform(-0.45, 0.45, NVIS)
        self.wb = rng.integers(0, W, NVIS)
        # the visibilities the edits move: a known cell (40 right / 25 up of the centre), 0.3 of a cell into it -> slice 1
        for k in (0, NVIS - 1):
            self.u[k] = 40.3 / N
            self.v[k] = 25.3 / N
            self.wb[k] = 2
        self.vis = rng.normal(size=NVIS) + 1j * rng.normal(size=NVIS)
        self.vis2 = rng.normal(size=NVIS) + 1j * rng.normal(size=NVIS)
        self.oracle = oracle
        self.ref = self.grid_ref(self.u, self.v, self.wb, self.vis)

    def grid_ref(self, u, v, wb, vis, gcf=None, n=N):
        gcf = self.gcf if gcf is None else gcf
        return self.oracle.convgrid2(gcf, np.zeros((n, n), dtype=np.complex128), u, v, wb, vis, mt_mode=2)

    def one(self, k, u, v, wb):
        """what visibility k adds to the grid at coordinates (u, v, wb)"""
        return self.grid_ref(np.array([u]), np.array([v]), np.array([wb]), self.vis[k:k + 1])


_bases = {}


@pytest.fixture(params=[7, 15, 17], ids=lambda S: f"S{S}")
def base(oracle, request):
    S = request.param
    if S not in _bases:
        _bases[S] = Base(oracle, S)
    return _bases[S]


@pytest.fixture
def rctx():
    """A context of its own, so that the counters start at zero and no other test's state is in it."""
    import gridhip
    c = gridhip.Context(0)
    c.set_option("prepass", 2)
    c.set_option("sort", 1)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def counters(c):
    import torch
    torch.cuda.synchronize()
    c.synchronize()
    return c.get_option("prepass_verified"), c.get_option("prepass_reused")


def grid(c, gcf, u, v, wb, vis, n=N):
    import torch
    G = torch.zeros((n, n), dtype=torch.complex128, device="cuda:0")
    c.convgrid2(gcf, G, (u, v, None), wb, vis)
    torch.cuda.synchronize()
    assert c.get_option("errors") == 0
    return G.cpu().numpy()


def test_values_only_change(rctx, base):
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    g1 = grid(rctx, gcf, u, v, wb, dev(b.vis))
    assert counters(rctx) == (0, 0)
    g2 = grid(rctx, gcf, u, v, wb, dev(b.vis2))
    assert counters(rctx) == (1, 1)
    assert rctx.last_dropped() == 0
    assert rel(g1, b.ref) < TOL
    assert rel(g2, b.grid_ref(b.u, b.v, b.wb, b.vis2)) < TOL


def test_dropped_visibilities_are_counted_and_zeroed_on_reuse(rctx, base):
    """what the skipped counting sweep did besides counting bins: the dropped count and a degrid's zeros"""
    import torch
    b = base
    wbn, un = b.wb.copy(), b.u.copy()
    wbn[::997] = W + 1
    wbn[5::1009] = -1
    un[7::1013] = 0.9  # no tap in the grid: dropped, not counted
    keep = (wbn >= 0) & (wbn < W) & (un < 0.6)
    ref = b.grid_ref(un[keep], b.v[keep], wbn[keep], b.vis[keep])
    gcf, u, v, wb, vis = dev(b.gcf), dev(un), dev(b.v), dev(wbn), dev(b.vis)
    g1 = grid(rctx, gcf, u, v, wb, vis)
    d1 = rctx.last_dropped()
    g2 = grid(rctx, gcf, u, v, wb, vis)
    assert counters(rctx) == (1, 1)
    assert rctx.last_dropped() == d1 == int(((wbn < 0) | (wbn >= W)).sum())
    assert rel(g1, ref) < TOL and rel(g2, ref) < TOL
    out = torch.full((NVIS,), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    rctx.degrid2(gcf, dev(ref), (u, v, None), wb, out)
    assert counters(rctx) == (2, 2)
    d = out.cpu().numpy()
    assert np.all(d[~keep] == 0) and rctx.last_dropped() == d1
    dref = b.oracle.degrid2(b.gcf, ref, un[keep], b.v[keep], wbn[keep])
    assert rel(d[keep], dref) < TOL


# (field, new value or function of the old one, kept?)  u = 40.3 / N sits in slice 1 of its cell; + 0.25 / N is slice 2
EDITS = {
    "other_tile": ("u", lambda x: x + 96.0 / N, True),
    "same_cell_other_slice": ("u", lambda x: x + 0.25 / N, True),
    "same_cell_other_slice_v": ("v", lambda x: x - 0.25 / N, True),
    "out_of_range": ("u", lambda x: 0.9, False),
    "nan": ("v", lambda x: float("nan"), False),
    "other_plane_same_group": ("wb", lambda x: 3, True),
    "plane_too_high": ("wb", lambda x: W, False),
    "plane_negative": ("wb", lambda x: -1, False),
}


@pytest.mark.parametrize("k", [0, NVIS - 1], ids=["first", "last"])
@pytest.mark.parametrize("edit", list(EDITS))
def test_one_coordinate_edited_in_place(rctx, base, edit, k):
    b = base
    field, fn, kept = EDITS[edit]
    gcf, vis = dev(b.gcf), dev(b.vis)
    t = {"u": dev(b.u), "v": dev(b.v), "wb": dev(b.wb)}
    g1 = grid(rctx, gcf, t["u"], t["v"], t["wb"], vis)
    assert rel(g1, b.ref) < TOL
    old = {"u": b.u[k], "v": b.v[k], "wb": int(b.wb[k])}
    new = dict(old)
    new[field] = fn(old[field])
    t[field][k] = new[field]
    g2 = grid(rctx, gcf, t["u"], t["v"], t["wb"], vis)
    assert counters(rctx) == (1, 0), "verified once, not reused"
    ref = b.ref - b.one(k, old["u"], old["v"], old["wb"])
    if kept:
        ref = ref + b.one(k, new["u"], new["v"], new["wb"])
    assert rel(g2, ref) < TOL
    assert rctx.last_dropped() == (1 if edit.startswith("plane_") else 0)
    # the next call (which does not verify: back-off after the failed attempt) is right as well
    g3 = grid(rctx, gcf, t["u"], t["v"], t["wb"], vis)
    assert rel(g3, ref) < TOL


@pytest.mark.parametrize("k", [0, NVIS - 1], ids=["first", "last"])
def test_an_edit_that_changes_no_pre_record(rctx, base, k):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    grid(rctx, gcf, u, v, wb, vis)
    u[k] = float(np.nextafter(b.u[k], 1.0))  # the last bit: same cell, same slice
    g2 = grid(rctx, gcf, u, v, wb, vis)
    assert counters(rctx)[0] == 1  # (it may reuse, and does)
    assert rel(g2, b.ref) < TOL


def test_key_changes(rctx, base, oracle):
    import torch
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    rng = np.random.default_rng(5)

    def again():  # the base call: right, and never a reuse after a call under another key
        r0 = counters(rctx)[1]
        assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
        assert counters(rctx)[1] == r0

    again()
    # another grid size
    assert rel(grid(rctx, gcf, u, v, wb, vis, n=384), b.grid_ref(b.u, b.v, b.wb, b.vis, n=384)) < TOL
    again()
    # another support, another Q
    for (q, s) in ((Q, 9), (2, b.S)):
        k2 = rng.normal(size=(W, q, q, s, s)) + 1j * rng.normal(size=(W, q, q, s, s))
        assert rel(grid(rctx, dev(k2), u, v, wb, vis), b.grid_ref(b.u, b.v, b.wb, b.vis, gcf=k2)) < TOL
        again()
    # options that shape the bins or the work items
    for key, val in (("wgroups", 2), ("tile", 32), ("chunk", 1024)):
        rctx.set_option(key, val)
        try:
            assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
        finally:
            rctx.set_option(key, 0)
        again()
    # a prefix of the stream
    m = NVIS - 4097
    assert rel(grid(rctx, gcf, u[:m], v[:m], wb[:m], vis[:m]), b.grid_ref(b.u[:m], b.v[:m], b.wb[:m], b.vis[:m])) < TOL
    again()
    assert counters(rctx)[1] == 0
    # a strided view of the same coordinates: its own key (and it reuses under it)
    uvw = torch.stack([u, v, torch.zeros_like(u)], dim=1).contiguous()
    for i in range(2):
        G = torch.zeros((N, N), dtype=torch.complex128, device="cuda:0")
        rctx.convgrid2(gcf, G, uvw, wb, vis)
        assert rel(G.cpu().numpy(), b.ref) < TOL
        assert counters(rctx)[1] == i
    again()


def test_intervening_writers(rctx, base, oracle):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    rng = np.random.default_rng(6)
    n_big = NVIS + (1 << 17)
    big = (rng.uniform(-0.45, 0.45, n_big), rng.uniform(-0.45, 0.45, n_big), rng.integers(0, W, n_big),
           rng.normal(size=n_big) + 1j * rng.normal(size=n_big))

    def aw():
        S, A, n = 7, 4, 300
        wk = rng.normal(size=(2, 2, 2, S, S)) + 1j * rng.normal(size=(2, 2, 2, S, S))
        ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
        rctx.convgrid4(wk, ak, np.zeros((64, 64), dtype=np.complex128), (rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), None),
                       (rng.integers(0, 2, n), rng.integers(0, A, n), rng.integers(0, A, n)),
                       rng.normal(size=n) + 1j * rng.normal(size=n))

    def plan():
        p = rctx.plan((N, N), b.gcf.shape, (u, v, None), wb)
        del p

    def degrid_elsewhere():
        rctx.degrid2(gcf, dev(b.ref), (dev(b.v), dev(b.u), None), dev(b.wb))

    def one_level():
        rctx.set_option("prepass", 1)
        try:
            assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
        finally:
            rctx.set_option("prepass", 2)

    def larger():
        got = grid(rctx, gcf, dev(big[0]), dev(big[1]), dev(big[2]), dev(big[3]))
        assert rel(got, b.grid_ref(*big)) < TOL

    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    for writer in (aw, plan, degrid_elsewhere, one_level, larger):
        writer()
        assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL, writer.__name__
        assert counters(rctx)[1] == 0, writer.__name__
    # (and with nothing in between it does reuse)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx)[1] == 1


@pytest.mark.parametrize("order", ["degrid_first", "grid_first"])
def test_gridding_and_degridding_share(rctx, base, order):
    """<g, grid(vis)> == <degrid_{conj K}(g), vis> (tests/test_gpu_parity.py: 1e-11), the second pass on kept records"""
    import torch
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    g = np.random.default_rng(2).normal(size=(N, N)) + 1j * np.random.default_rng(3).normal(size=(N, N))
    cg, dg = dev(np.conj(b.gcf)), dev(g)

    def degrid():
        d = rctx.degrid2(cg, dg, (u, v, None), wb)
        torch.cuda.synchronize()
        return d.cpu().numpy()

    if order == "degrid_first":
        d = degrid()
        G = grid(rctx, gcf, u, v, wb, vis)
    else:
        G = grid(rctx, gcf, u, v, wb, vis)
        d = degrid()
    assert counters(rctx) == (1, 1)
    assert rctx.get_option("errors") == 0
    assert rel(G, b.ref) < TOL
    lhs, rhs = np.vdot(g, G), np.vdot(d, b.vis)
    assert abs(lhs - rhs) / abs(lhs) < 1e-11


def test_bin_reuse_1_never_verifies(rctx, base):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    rctx.set_option("bin_reuse", 1)
    for _ in range(3):
        assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx) == (0, 0)
    rctx.set_option("bin_reuse", 0)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx) == (1, 1)


def test_back_off_after_a_failed_attempt(rctx, base):
    """the same arrays with new contents before every call: verified once, then not for 4 calls, then tried again"""
    import torch
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    rng = np.random.default_rng(8)
    seen = []
    for call in range(8):
        hu = rng.uniform(-0.45, 0.45, NVIS)
        u.copy_(torch.from_numpy(hu))
        got = grid(rctx, gcf, u, v, wb, vis)
        seen.append(counters(rctx))
    assert [s[0] for s in seen] == [0, 1, 1, 1, 1, 1, 2, 2]
    assert all(s[1] == 0 for s in seen)
    assert rel(got, b.grid_ref(hu, b.v, b.wb, b.vis)) < TOL


@pytest.mark.parametrize("held", ["one_level_elsewhere", "two_level_prefix"])
def test_replayed_graph_between_calls(rctx, base, held):
    """A graph captured earlier and replayed between two calls rewrites the records and tables (and, the two-level
    one, the pre-records of a prefix with the values they had) without entering the library: the call after it must
    not reuse, and is right."""
    import torch
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    if held == "one_level_elsewhere":  # a small launch-bound call on other arrays and another grid
        rng = np.random.default_rng(9)
        m, n = 20000, 128
        hu, hv, hw = rng.uniform(-0.4, 0.4, m), rng.uniform(-0.4, 0.4, m), rng.integers(0, W, m)
        hvis = rng.normal(size=m) + 1j * rng.normal(size=m)
        prepass = 1
    else:
        m, n = NVIS - 4097, N
        hu, hv, hw, hvis = b.u[:m], b.v[:m], b.wb[:m], b.vis[:m]
        prepass = 2
    href = b.grid_ref(hu, hv, hw, hvis, n=n)
    du, dv, dw, dvis = (u[:m], v[:m], wb[:m], vis[:m]) if prepass == 2 else (dev(hu), dev(hv), dev(hw), dev(hvis))
    HG = torch.zeros((n, n), dtype=torch.complex128, device="cuda:0")
    # the largest call first: a graph holds the addresses of the scratch blocks, which must not grow after the capture
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    rctx.set_option("prepass", prepass)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            rctx.convgrid2(gcf, HG, (du, dv, None), dw, dvis)  # warm-up on the capture stream
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            rctx.convgrid2(gcf, HG, (du, dv, None), dw, dvis)
        torch.cuda.synchronize()
    finally:
        rctx.set_option("prepass", 2)
    v0, r0 = counters(rctx)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx) == (v0 + 1, r0 + 1)  # (eager calls with nothing in between do reuse)
    HG.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert rel(HG.cpu().numpy(), href) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx)[1] == r0 + 1, "no reuse after a replay"
    # a replay straight after the call that would keep state, then the values change
    graph.replay()
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.grid_ref(b.u, b.v, b.wb, b.vis2)) < TOL
    assert counters(rctx)[1] == r0 + 1
