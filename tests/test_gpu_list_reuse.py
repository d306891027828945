"""The tap-reusing tile kernel keeps each work item's slice-sorted list when the pre-pass keeps its records
(csrc/tile_sorted.hip, "Kept lists").

A plain convgrid2 / degrid2 over the two-level pre-pass sorts into one per-call array, a work item's list at the
position of its records.  The next such call under the same geometry and the next pre-pass generation is told by the
host that the lists are there (`lists_reused` counts those launches), and the kernel walks them without sorting if the
verify sweep's verdict says the records stand (`prepass_reused` counts those).  Checked here: values-only changes walk
kept lists and give each call's own result; gridding and degridding share one set; an edited coordinate makes the
kernel sort afresh whatever the host said, and the new lists are reused once the pre-pass verifies again (it pauses for
4 calls after a failed attempt, tests/test_gpu_bin_reuse.py); a changed work-item shape or an intervening writer never
reuses; short items, ragged counts, mostly empty queues and short-lived work-groups (`yield_cus`) walk kept lists
correctly; `list_reuse` = 1 and `bin_reuse` = 1 switch it off.

Shapes, streams and tolerance are those of tests/test_gpu_bin_reuse.py: 2^18 visibilities forced onto the two-level
path and the tap-reusing kernel (prepass = 2, sort = 1), a 512^2 grid, 8 planes, Q = 4, supports 7, 15 and 17 (17: the
tap list in parts), parity against oracle.gridref_c at 1e-10 relative (fp64 atomics reorder sums), `errors` == 0 after
every call.
"""
import numpy as np
import pytest

from test_gpu_bin_reuse import Base, N, NVIS, Q, TOL, W, dev, rel

pytestmark = pytest.mark.gpu

_bases = {}


class ListBase(Base):
    """The stream of tests/test_gpu_bin_reuse.py plus the further oracle results these tests compare with, each
    computed once."""

    def __init__(self, oracle, S):
        super().__init__(oracle, S)
        self._ref2 = self._dref = None
        self.model = np.random.default_rng(2).normal(size=(N, N)) + 1j * np.random.default_rng(3).normal(size=(N, N))

    @property
    def ref2(self):
        if self._ref2 is None:
            self._ref2 = self.grid_ref(self.u, self.v, self.wb, self.vis2)
        return self._ref2

    @property
    def dref(self):
        if self._dref is None:
            self._dref = self.oracle.degrid2(self.gcf, self.model, self.u, self.v, self.wb)
        return self._dref


@pytest.fixture(params=[7, 15, 17], ids=lambda S: f"S{S}")
def base(oracle, request):
    S = request.param
    if S not in _bases:
        _bases[S] = ListBase(oracle, S)
    return _bases[S]


@pytest.fixture
def rctx():
    import gridhip
    c = gridhip.Context(0)
    c.set_option("prepass", 2)
    c.set_option("sort", 1)
    yield c
    c.close()


def counters(c):
    """(calls that kept their records, tile launches told to trust the kept lists)"""
    import torch
    torch.cuda.synchronize()
    c.synchronize()
    return c.get_option("prepass_reused"), c.get_option("lists_reused")


def grid(c, gcf, u, v, wb, vis, n=N):
    import torch
    G = torch.zeros((n, n), dtype=torch.complex128, device="cuda:0")
    c.convgrid2(gcf, G, (u, v, None), wb, vis)
    torch.cuda.synchronize()
    assert c.get_option("errors") == 0
    return G.cpu().numpy()


def degrid(c, gcf, model, u, v, wb):
    import torch
    out = torch.full((u.shape[0],), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    c.degrid2(gcf, model, (u, v, None), wb, out)
    torch.cuda.synchronize()
    assert c.get_option("errors") == 0
    return out.cpu().numpy()


def test_values_only_change(rctx, base):
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    g1 = grid(rctx, gcf, u, v, wb, dev(b.vis))
    assert counters(rctx) == (0, 0)
    assert rctx.get_option("last_path") == 1  # the tap-reusing kernel, one record per visibility
    g2 = grid(rctx, gcf, u, v, wb, dev(b.vis2))
    assert counters(rctx) == (1, 1)
    g3 = grid(rctx, gcf, u, v, wb, dev(b.vis))
    assert counters(rctx) == (2, 2)
    assert rel(g1, b.ref) < TOL
    assert rel(g2, b.ref2) < TOL
    assert rel(g3, b.ref) < TOL


@pytest.mark.parametrize("order", ["grid_first", "degrid_first"])
def test_gridding_and_degridding_share_lists(rctx, base, order):
    b = base
    gcf, u, v, wb, vis, model = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis), dev(b.model)
    seq = ["g", "d", "g"] if order == "grid_first" else ["d", "g", "d"]
    for i, what in enumerate(seq):
        if what == "g":
            assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL, i
        else:
            assert rel(degrid(rctx, gcf, model, u, v, wb), b.dref) < TOL, i
        assert counters(rctx) == (i, i)


@pytest.mark.parametrize("k", [0, NVIS - 1], ids=["first", "last"])
def test_one_coordinate_edited_in_place(rctx, base, k):
    """The host cannot know that the stream changed: it tells the launch the lists are valid (the counter moves), the
    verdict on the device says otherwise and the kernel sorts the rewritten records.  The pre-pass then pauses for 4
    calls; the first call that verifies again walks the lists the call before it wrote."""
    b = base
    gcf, vis = dev(b.gcf), dev(b.vis)
    u, v, wb = dev(b.u), dev(b.v), dev(b.wb)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    new_u = b.u[k] + 96.0 / N  # another tile
    u[k] = new_u
    ref = b.ref - b.one(k, b.u[k], b.v[k], int(b.wb[k])) + b.one(k, new_u, b.v[k], int(b.wb[k]))
    assert rel(grid(rctx, gcf, u, v, wb, vis), ref) < TOL
    assert counters(rctx) == (0, 1), "told to reuse, records rewritten: sorted afresh"
    for _ in range(4):  # (back-off: no verify sweep, so no verdict to trust lists by)
        assert rel(grid(rctx, gcf, u, v, wb, vis), ref) < TOL
        assert counters(rctx) == (0, 1)
    assert rel(grid(rctx, gcf, u, v, wb, vis), ref) < TOL
    assert counters(rctx) == (1, 2), "the new lists are reused"
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2 - _moved(b, k, new_u, b.vis2)) < TOL
    assert counters(rctx) == (2, 3)


def _moved(b, k, new_u, vis):
    """what moving visibility k to new_u takes from the base grid of `vis` (old contribution minus new one)"""
    one = lambda uu: b.oracle.convgrid2(b.gcf, np.zeros((N, N), dtype=np.complex128), np.array([uu]), b.v[k:k + 1],
                                        b.wb[k:k + 1], vis[k:k + 1], mt_mode=2)
    return one(b.u[k]) - one(new_u)


@pytest.mark.parametrize("k", [0, NVIS - 1], ids=["first", "last"])
def test_an_edit_that_changes_no_pre_record(rctx, base, k):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    grid(rctx, gcf, u, v, wb, vis)
    u[k] = float(np.nextafter(b.u[k], 1.0))  # the last bit: same cell, same slice
    g2 = grid(rctx, gcf, u, v, wb, vis)
    assert counters(rctx) == (1, 1)
    assert rel(g2, b.ref) < TOL


def test_work_item_shape_changes(rctx, base):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    for key, val in (("chunk", 1024), ("wgroups", 2), ("tile", 32)):
        rctx.set_option(key, val)
        try:
            assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL, key
        finally:
            rctx.set_option(key, 0)
        assert counters(rctx) == (0, 0), key
        assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL, key
        assert counters(rctx) == (0, 0), key
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2) < TOL
    assert counters(rctx) == (1, 1)


def test_short_items(rctx, base):
    """chunk = 64: many work items per bin, every one at most a block of the walk"""
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    rctx.set_option("chunk", 64)
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis)), b.ref) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2) < TOL
    assert rel(degrid(rctx, gcf, dev(b.model), u, v, wb), b.dref) < TOL
    assert counters(rctx) == (2, 2)


@pytest.mark.parametrize("chunk", [0, 64])
def test_ragged_count_in_a_few_tiles(rctx, base, chunk):
    """a visibility count that is no multiple of 64, confined to a few tiles: most queues are empty"""
    b = base
    m = 50001
    rng = np.random.default_rng(77)
    hu, hv = rng.uniform(0.05, 0.12, m), rng.uniform(-0.2, -0.15, m)
    hw = b.wb[:m]
    ref1, ref2 = b.grid_ref(hu, hv, hw, b.vis[:m]), b.grid_ref(hu, hv, hw, b.vis2[:m])
    gcf, u, v, wb = dev(b.gcf), dev(hu), dev(hv), dev(hw)
    rctx.set_option("chunk", chunk)
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis[:m])), ref1) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2[:m])), ref2) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis[:m])), ref1) < TOL
    assert counters(rctx) == (2, 2)


def test_intervening_writers(rctx, base):
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    rng = np.random.default_rng(6)

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

    def one_level():
        rctx.set_option("prepass", 1)
        try:
            assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
        finally:
            rctx.set_option("prepass", 2)

    def other_grid_size():
        assert rel(grid(rctx, gcf, u, v, wb, vis, n=384), b.grid_ref(b.u, b.v, b.wb, b.vis, n=384)) < TOL

    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    for writer in (plan, aw, one_level, other_grid_size):
        writer()
        assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL, writer.__name__
        assert counters(rctx) == (0, 0), writer.__name__
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2) < TOL
    assert counters(rctx) == (1, 1)


@pytest.mark.parametrize("held", ["one_level_elsewhere", "two_level_prefix"])
def test_replayed_graph_between_calls(rctx, base, held):
    """A replay of a graph captured earlier (set up as in tests/test_gpu_bin_reuse.py) rewrites records and tables -
    the two-level one also the head of the block the lists live in - without entering the library.  The host still
    tells the next launch that the lists are valid; the verdict the replay disarmed makes the kernel sort."""
    import torch
    b = base
    gcf, u, v, wb, vis = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb), dev(b.vis)
    if held == "one_level_elsewhere":
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
    r0, l0 = counters(rctx)
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx) == (r0, l0), "the captured call left no lists"
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL
    assert counters(rctx) == (r0 + 1, l0 + 1)
    HG.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert rel(HG.cpu().numpy(), href) < TOL
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2) < TOL
    assert counters(rctx)[0] == r0 + 1, "no reuse after a replay"
    assert rel(grid(rctx, gcf, u, v, wb, vis), b.ref) < TOL  # (back-off: a full pre-pass, a fresh sort)
    assert counters(rctx)[0] == r0 + 1


def test_list_reuse_1_never_reuses(rctx, base):
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    rctx.set_option("list_reuse", 1)
    for vis, ref in ((b.vis, b.ref), (b.vis2, b.ref2), (b.vis, b.ref)):
        assert rel(grid(rctx, gcf, u, v, wb, dev(vis)), ref) < TOL
    assert counters(rctx) == (2, 0)
    rctx.set_option("list_reuse", 0)
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis2)), b.ref2) < TOL
    assert counters(rctx) == (3, 0), "the call before kept no lists"
    assert rel(grid(rctx, gcf, u, v, wb, dev(b.vis)), b.ref) < TOL
    assert counters(rctx) == (4, 1)


def test_bin_reuse_1_never_reuses(rctx, base):
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    rctx.set_option("bin_reuse", 1)
    for vis, ref in ((b.vis, b.ref), (b.vis2, b.ref2), (b.vis, b.ref)):
        assert rel(grid(rctx, gcf, u, v, wb, dev(vis)), ref) < TOL
    assert counters(rctx) == (0, 0)


def test_short_lived_work_groups(rctx, base):
    """yield_cus: work-groups that take eight items and leave share the per-position array with the persistent ones"""
    b = base
    gcf, u, v, wb = dev(b.gcf), dev(b.u), dev(b.v), dev(b.wb)
    rctx.set_option("yield_cus", 32)
    rctx.set_option("chunk", 256)  # (enough work items for the short-lived work-groups to exist)
    for i, (vis, ref) in enumerate(((b.vis, b.ref), (b.vis2, b.ref2), (b.vis, b.ref))):
        assert rel(grid(rctx, gcf, u, v, wb, dev(vis)), ref) < TOL
        assert counters(rctx) == (i, i)
    assert rel(degrid(rctx, gcf, dev(b.model), u, v, wb), b.dref) < TOL
    assert counters(rctx) == (3, 3)
