"""The verify sweep of the pre-pass reuse compares digests, not pre-records (csrc/bin.hip "Reuse", csrc/bin_digest.h).

The counting sweep keeps one 128-bit digest per aligned group of 128 consecutive pre-records; a later call over the same
arrays derives every pre-record again, adds up the digest contributions and keeps its records if the sums are the kept
ones.  Checked here, at the group and pair edges of the sweep's index space: values-only changes reuse; one edited
coordinate (a whole cell in u or v, one sub-cell in u, the plane) at the first, middle and last places of a group
does not, nor do two visibilities that swap their coordinates - inside one thread's pair, at the two ends of a group,
across two groups - and the grid is then the oracle's of the edited stream; an edit that leaves the pre-record as it
was reuses; a dropped visibility is counted, and its prediction zeroed, by the reused call as well; gridding and
degridding share the state.

Shapes: contexts as in tests/test_gpu_bin_reuse.py (prepass = 2, sort = 1), a 256^2 grid, 4 planes, Q = 4, support 7
at n in {1, 2, 127, 128, 129, 255, 257, 16385} (16385: more than one trip of a work-group) and support 17 (the kernel
in parts: the one-element forms of both sweeps) at n = 257; arrays 8 bytes off a 16-byte boundary take the one-element
forms at support 7.  Every coordinate sits 0.3 of a cell into its cell (sub-cell 1 of 4), so a move by a quarter cell
changes the slice alone and one by 1e-9 cells changes nothing, on the CPU oracle as on the device.  Parity is against
oracle.gridref_c.convgrid2 at 1e-10 relative, as in the existing reuse tests (fp64 atomics reorder sums).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10
N, W, Q = 256, 4, 4
NS = [1, 2, 127, 128, 129, 255, 257, 16385]
SHAPES = [(7, n) for n in NS] + [(17, 257)]
EDIT_AT = [0, 63, 64, 126, 127, 128, -1]
SWAPS = {"one_pair": (2, 3), "group_ends": (0, 127), "across_groups": (127, 128)}


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Base:
    """One seeded stream per (support, n), its kernel table and the oracle's grid of it (computed once, never changed)."""

    def __init__(self, oracle, S, n):
        rng = np.random.default_rng(7000 + 100 * S + n)
        self.S, self.n, self.oracle = S, n, oracle
        self.gcf = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
        self.u = (rng.integers(-100, 101, n) + 0.3) / N
        self.v = (rng.integers(-100, 101, n) + 0.3) / N
        self.wb = rng.integers(0, W, n)
        # the places the swaps use: known, pairwise different cells and planes
        for k in {i for pair in SWAPS.values() for i in pair}:
            if k < n:
                self.u[k] = ((7 * k) % 150 - 75 + 0.3) / N
                self.v[k] = (80 - 5 * (k % 29) + 0.3) / N
                self.wb[k] = k % W
        self.vis = rng.normal(size=n) + 1j * rng.normal(size=n)
        self.vis2 = rng.normal(size=n) + 1j * rng.normal(size=n)
        self.ref = self.grid_ref(self.u, self.v, self.wb, self.vis)

    def grid_ref(self, u, v, wb, vis):
        return self.oracle.convgrid2(self.gcf, np.zeros((N, N), dtype=np.complex128), u, v, wb, vis, mt_mode=2)


_bases = {}


def get_base(oracle, S, n):
    if (S, n) not in _bases:
        _bases[(S, n)] = Base(oracle, S, n)
    return _bases[(S, n)]


def shape_id(p):
    return f"S{p[0]}-n{p[1]}" + ("-off8" if len(p) > 2 and p[2] else "")


@pytest.fixture(params=SHAPES, ids=shape_id)
def base(oracle, request):
    return get_base(oracle, *request.param)


# (support, n, off): off = 1 puts the arrays 8 bytes past a 16-byte boundary - the one-element forms at support 7
VALUE_SHAPES = [(S, n, 0) for S, n in SHAPES] + [(7, 129, 1), (7, 16385, 1)]
SWAP_CASES = [(S, n, 0, name) for S, n in SHAPES for name, (_, j) in SWAPS.items() if j < n] + [(7, 257, 1, name) for name in SWAPS]


@pytest.fixture
def rctx():
    """A context of its own, so that the counters start at zero and no other test's state is in it."""
    import gridhip
    c = gridhip.Context(0)
    c.set_option("prepass", 2)
    c.set_option("sort", 1)
    yield c
    c.close()


def dev(a, off=0):
    """`a` on the device; off = 1: 8 bytes past a 16-byte boundary (the sweeps' one-element forms)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to("cuda:0")
    full = torch.empty(len(a) + 2, dtype=t.dtype, device="cuda:0")
    start = 1 if full.data_ptr() % 16 == 0 else 2
    full[start:start + len(a)] = t.to("cuda:0")
    return full[start:start + len(a)]


def counters(c):
    import torch
    torch.cuda.synchronize()
    c.synchronize()
    return c.get_option("prepass_verified"), c.get_option("prepass_reused")


def grid(c, gcf, u, v, wb, vis):
    import torch
    G = torch.zeros((N, N), dtype=torch.complex128, device="cuda:0")
    c.convgrid2(gcf, G, (u, v, None), wb, vis)
    torch.cuda.synchronize()
    assert c.get_option("errors") == 0
    return G.cpu().numpy()


class Stream:
    """A copy of the base stream on the device under addresses of its own (every copy of a test stays alive, so no two
    share an address and each starts under a new key), with its host mirror."""

    alive = []

    def __init__(self, b, off=0):
        self.h = {"u": b.u.copy(), "v": b.v.copy(), "wb": b.wb.copy()}
        self.d = {f: dev(a, off) for f, a in self.h.items()}
        Stream.alive.append(self)

    def set(self, field, k, value):
        self.h[field][k] = value
        self.d[field][k] = value

    def args(self):
        return self.d["u"], self.d["v"], self.d["wb"]

    def host(self):
        return self.h["u"], self.h["v"], self.h["wb"]


@pytest.fixture(autouse=True)
def _drop_streams():
    yield
    Stream.alive.clear()


@pytest.mark.parametrize("shape", VALUE_SHAPES, ids=shape_id)
def test_values_change_only(rctx, oracle, shape):
    b, off = get_base(oracle, shape[0], shape[1]), shape[2]
    gcf, s = dev(b.gcf), Stream(b, off)
    g1 = grid(rctx, gcf, *s.args(), dev(b.vis))
    assert counters(rctx) == (0, 0)
    g2 = grid(rctx, gcf, *s.args(), dev(b.vis2))
    assert counters(rctx) == (1, 1)
    assert rctx.last_dropped() == 0
    assert rel(g1, b.ref) < TOL
    assert rel(g2, b.grid_ref(b.u, b.v, b.wb, b.vis2)) < TOL


EDITS = {
    "u_whole_cell": ("u", lambda x: x + 1.0 / N),
    "u_one_sub_cell": ("u", lambda x: x + 0.25 / N),
    "v_whole_cell": ("v", lambda x: x + 1.0 / N),
    "plane": ("wb", lambda x: (x + 1) % W),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_one_coordinate_edited(rctx, base, edit):
    b = base
    field, fn = EDITS[edit]
    gcf, vis = dev(b.gcf), dev(b.vis)
    places = sorted({k % b.n for k in EDIT_AT if k < b.n})
    for k in places:
        s = Stream(b)
        v0, r0 = counters(rctx)
        g1 = grid(rctx, gcf, *s.args(), vis)
        assert counters(rctx) == (v0, r0), "a new stream: nothing to verify"
        assert rel(g1, b.ref) < TOL
        old = s.h[field][k]
        s.set(field, k, int(fn(old)) if field == "wb" else float(fn(old)))
        g2 = grid(rctx, gcf, *s.args(), vis)
        assert counters(rctx) == (v0 + 1, r0), f"element {k}: verified once, not reused"
        assert rel(g2, b.grid_ref(*s.host(), b.vis)) < TOL, f"element {k}"
        assert rctx.last_dropped() == 0


@pytest.mark.parametrize("case", SWAP_CASES, ids=lambda c: shape_id(c) + "-" + c[3])
def test_two_visibilities_swap_their_coordinates(rctx, oracle, case):
    b, off = get_base(oracle, case[0], case[1]), case[2]
    i, j = SWAPS[case[3]]
    gcf, vis, s = dev(b.gcf), dev(b.vis), Stream(b, off)
    assert rel(grid(rctx, gcf, *s.args(), vis), b.ref) < TOL
    assert b.vis[i] != b.vis[j]
    for f in ("u", "v", "wb"):
        assert s.h[f][i] != s.h[f][j]
        a, c = s.h[f][i].item(), s.h[f][j].item()
        s.set(f, i, c)
        s.set(f, j, a)
    g2 = grid(rctx, gcf, *s.args(), vis)
    assert counters(rctx) == (1, 0), "verified once, not reused"
    ref = b.grid_ref(*s.host(), b.vis)
    assert rel(ref, b.ref) > 1e-6  # (the swap does change the grid)
    assert rel(g2, ref) < TOL


def test_an_edit_that_leaves_the_pre_record(rctx, base):
    b = base
    gcf, vis = dev(b.gcf), dev(b.vis)
    v0 = r0 = 0
    for k in sorted({k % b.n for k in EDIT_AT if k < b.n}):
        s = Stream(b)
        grid(rctx, gcf, *s.args(), vis)
        s.set("u", k, float(s.h["u"][k] + 1e-9 / N))  # inside its sub-cell
        g2 = grid(rctx, gcf, *s.args(), vis)
        v0, r0 = v0 + 1, r0 + 1
        assert counters(rctx) == (v0, r0), f"element {k}: reused"
        assert rel(g2, b.grid_ref(*s.host(), b.vis)) < TOL


@pytest.mark.parametrize("how", ["no_tap_in_the_grid", "plane_out_of_range"])
def test_one_visibility_out_of_range_then_repeated(rctx, base, how):
    import torch
    b = base
    k = b.n // 2
    gcf, vis, s = dev(b.gcf), dev(b.vis), Stream(b)
    if how == "no_tap_in_the_grid":
        s.set("u", k, 0.9)  # dropped, not counted
    else:
        s.set("wb", k, W)  # dropped and counted
    keep = np.arange(b.n) != k
    hu, hv, hw = s.host()
    ref = b.grid_ref(hu[keep], hv[keep], hw[keep], b.vis[keep]) if b.n > 1 else np.zeros((N, N), dtype=np.complex128)
    g1 = grid(rctx, gcf, *s.args(), vis)
    d1 = rctx.last_dropped()
    g2 = grid(rctx, gcf, *s.args(), vis)
    assert counters(rctx) == (1, 1)
    assert rctx.last_dropped() == d1 == (1 if how == "plane_out_of_range" else 0)
    assert rel(g1, ref) < TOL and rel(g2, ref) < TOL
    out = torch.full((b.n,), 7 + 7j, dtype=torch.complex128, device="cuda:0")
    rctx.degrid2(gcf, dev(ref), (s.d["u"], s.d["v"], None), s.d["wb"], out)
    assert counters(rctx) == (2, 2)
    d = out.cpu().numpy()
    assert d[k] == 0 and rctx.last_dropped() == d1
    if b.n > 1:
        dref = b.oracle.degrid2(b.gcf, ref, hu[keep], hv[keep], hw[keep])
        assert rel(d[keep], dref) < TOL


@pytest.mark.parametrize("order", ["degrid_first", "grid_first"])
def test_gridding_and_degridding_share(rctx, base, order):
    import torch
    b = base
    gcf, vis, s = dev(b.gcf), dev(b.vis), Stream(b)
    dg = dev(b.ref)

    def degrid():
        d = rctx.degrid2(gcf, dg, (s.d["u"], s.d["v"], None), s.d["wb"])
        torch.cuda.synchronize()
        return d.cpu().numpy()

    if order == "degrid_first":
        d = degrid()
        G = grid(rctx, gcf, *s.args(), vis)
    else:
        G = grid(rctx, gcf, *s.args(), vis)
        d = degrid()
    assert counters(rctx) == (1, 1)
    assert rctx.get_option("errors") == 0
    assert rel(G, b.ref) < TOL
    assert rel(d, b.oracle.degrid2(b.gcf, b.ref, b.u, b.v, b.wb)) < TOL
