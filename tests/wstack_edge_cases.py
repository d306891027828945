"""Inputs that test_wstack_edges_host.py (host) and test_gpu_wstack_edges.py (GPU) share: the streams at which w-stacking
(wstack.hip, idg.hip) meets plane ties, the seams of its partition, wide fields, the horizon, every width of the
image-domain degridder and degenerate streams.  No GPU: plain numpy and the restatements wstack_ref and idg_ref, which
are used as they are.  Every builder has a fixed seed and is computed once; its arrays are read-only.

A case is a dict: theta, lam, N, u, v, w, vis, model, fn (the tuple Context.wstack / do_imaging / predict take), ref (the
restatement's plan), image = ref.image(vis), pred = ref.predict(model), kept (the visibilities with a layer and, for
image-domain layers, a tile) and dropped (the others' number: what the device must count).

The device's own shapes that the cases are built around (wstack.hip, idg.hip):
  SCATTER  ws_scatter_kernel ranks 256 x 8 visibilities per work-group; a stream of more takes several work-groups, which
           hand their places in a layer's slice to each other through one global add per layer (`cursor`)
  SCAN     ws_scan_kernel is one work-group of 256 threads with ceil(L / 256) layers each
  SPLIT    a tile of more visibilities is cut into work items of this many (read-only option "idg_split")
  WIDTHS   idg_degrid_launch takes 64, 128 or 256 threads where the layer's mean item, nvis div nitems, is <= 64, <= 128, more"""
import functools

import numpy as np

import idg_ref as I
import wstack_ref as W
from oracle import gridref_np as R

WSTEP, NPIXFF = 100, 16
THETA48, LAM48 = 0.15, 320  # the default shape: N = 48, no multiple of a 16-cell tile
SCATTER, SCAN, SPLIT = 256 * 8, 256, 1024


def degrid_threads(mean):
    return 64 if mean <= 64 else 128 if mean <= 128 else 256


def wfn(M, S, Q, wstep=WSTEP):
    return ("wstack", dict(wstep=wstep, planes=M, qpx=Q, npixFF=NPIXFF, npixKern=S))


def ifn(sk, M, wstep=WSTEP):
    return ("idg", dict(wstep=wstep, planes=M, subgrid=sk[0], margin=sk[1]))


def build(fn, theta, lam, u, v, w, rng):
    """the case of a stream: vis and model from `rng`, the restatement's plan and its two outputs"""
    u, v, w = (np.ascontiguousarray(x, dtype=np.float64) for x in (u, v, w))
    n = len(u)
    N = W.image_size(theta, lam)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    model = rng.normal(size=(N, N))
    o = fn[1]
    if fn[0] == "idg":
        ref = I.Stack(theta, lam, u, v, w, o["wstep"], o["planes"], o["subgrid"], o["margin"])
        kept = ref.keep
    else:
        ref = W.Stack(theta, lam, u, v, w, o["wstep"], o["planes"], o["qpx"], o["npixFF"], o["npixKern"])
        kept = ref.lay["finite"]
    c = dict(theta=theta, lam=lam, N=N, n=n, u=u, v=v, w=w, vis=vis, model=model, fn=fn, ref=ref, kept=kept,
             dropped=int(n - kept.sum()), image=ref.image(vis), pred=ref.predict(model))
    for x in c.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def imaging(build_case, *args):
    """the restatement's do_imaging of a case -> (image, psf, pmax), computed once"""
    c = build_case(*args)
    o = c["fn"][1]
    a = (c["theta"], c["lam"], c["u"], c["v"], c["w"], c["vis"], o["wstep"], o["planes"])
    with np.errstate(invalid="ignore"):
        if c["fn"][0] == "idg":
            return I.do_imaging(*a, o["subgrid"], o["margin"])
        return W.do_imaging(*a, o["qpx"], o["npixFF"], o["npixKern"])


def uv(rng, n, lam, span=0.4):
    return rng.uniform(-span * lam, span * lam, n), rng.uniform(-span * lam, span * lam, n)


def spread_w(rng, n, M, L, wstep=WSTEP):
    """w whose planes span exactly L layers of M planes around 0, the lowest and the highest plane both taken (make_w of
    test_gpu_wstack.py)"""
    span = L * M - 1
    pmin = -(span // 2)
    w = rng.uniform(pmin * wstep, (pmin + span) * wstep, n)
    w[0], w[1] = pmin * wstep, (pmin + span) * wstep
    return w


# ---- T: plane ties ------------------------------------------------------------------------------------------------------
def tie_w():
    """w = (k + 1/2) wstep for k = -7 .. 6, twelve each: every one a tie, which libm round takes away from zero (planes
    -7 .. -1 and 1 .. 7) and rint to the even plane (-6 .. 6).  Then the doubles next to 50 and 250 towards 0 and their
    negatives: w / wstep is below the tie, so they round to 0, 2, -0 and -2 (floor(x + 1/2) would make 1 of the first)."""
    k = np.repeat(np.arange(-7, 7), 12)
    near = [np.nextafter(50.0, 0.0), np.nextafter(250.0, 0.0), np.nextafter(-50.0, 0.0), np.nextafter(-250.0, 0.0)]
    return np.concatenate([(k + 0.5) * WSTEP, near])


@functools.lru_cache(maxsize=None)
def ties(M):
    rng = np.random.default_rng(100 + M)
    w = rng.permutation(tie_w())
    u, v = uv(rng, len(w), LAM48)
    return build(wfn(M, 7, 2), THETA48, LAM48, u, v, w, rng)


@functools.lru_cache(maxsize=None)
def ties_idg():
    rng = np.random.default_rng(110)
    w = rng.permutation(tie_w())
    u, v = uv(rng, len(w), LAM48)
    return build(ifn((16, 8), 2), THETA48, LAM48, u, v, w, rng)


class half_even:
    """inside: the restatement's plane rule is rint (ties to the even plane) instead of acc_round - the rule a device
    that rounds with rint would follow.  The restatement's file is not touched."""

    def __enter__(self):
        self.kept = R.acc_round
        R.acc_round = lambda x: np.rint(x).astype(np.int64)

    def __exit__(self, *exc):
        R.acc_round = self.kept


# ---- S: the scatter's seams ---------------------------------------------------------------------------------------------
SEAM_N = (2047, 2048, 2049, 6145)
SEAM_MSQ = ((1, 7, 2), (4, 7, 4))


@functools.lru_cache(maxsize=None)
def seam(n, msq):
    """n visibilities over 9 layers, all occupied: either side of one work-group of the scatter, and three and a bit"""
    rng = np.random.default_rng(200 + n)
    u, v = uv(rng, n, LAM48)
    return build(wfn(*msq), THETA48, LAM48, u, v, spread_w(rng, n, msq[0], 9), rng)


@functools.lru_cache(maxsize=None)
def one_plane():
    """4100 visibilities in plane 3: three work-groups, and every one adds to the same cursor"""
    rng = np.random.default_rng(210)
    n = 4100
    u, v = uv(rng, n, LAM48)
    return build(wfn(1, 7, 2), THETA48, LAM48, u, v, rng.uniform(260.0, 340.0, n), rng)


@functools.lru_cache(maxsize=None)
def every_layer():
    """6145 visibilities over 16 layers: every work-group of the scatter adds to every layer's cursor"""
    rng = np.random.default_rng(220)
    n = 6145
    u, v = uv(rng, n, LAM48)
    return build(wfn(1, 7, 2), THETA48, LAM48, u, v, spread_w(rng, n, 1, 16), rng)


IMAGER_SEAM = (65, (5, 9, 2), 16, 6145)  # (N, msq, L, n) of test_gpu_wstack_imager.against_the_calls


# ---- C: the scan's seams ------------------------------------------------------------------------------------------------
def scan_occupied(L):
    """257: every layer.  515: the layers l = 1 (mod 3) are empty - but for the last one, 514, which holds the highest plane
    (without it there are no 515 layers)."""
    return [l for l in range(L) if L == 257 or l % 3 != 1 or l == L - 1]


@functools.lru_cache(maxsize=None)
def scan(L):
    """M = 1, n = 2 L + 3: more layers than the scan has threads, so a thread takes 2 (L = 257: thread 128 takes the odd
    last one) or 3 (L = 515: thread 171 takes two) of them"""
    rng = np.random.default_rng(300 + L)
    n = 2 * L + 3
    occ = np.array(scan_occupied(L))
    p = np.concatenate([occ, rng.choice(occ, n - len(occ))]) - L // 2
    w = rng.permutation(p * float(WSTEP) + rng.uniform(-40.0, 40.0, n))
    u, v = uv(rng, n, LAM48)
    return build(wfn(1, 7, 2), THETA48, LAM48, u, v, w, rng)


# ---- F: wide fields -----------------------------------------------------------------------------------------------------
WIDE = {48: (1.2, 40), 65: (1.25, 52)}


@functools.lru_cache(maxsize=None)
def wide(N):
    theta, lam = WIDE[N]
    rng = np.random.default_rng(400 + N)
    n = 400
    u, v = uv(rng, n, lam)
    w = rng.uniform(-1500.0, 1500.0, n)
    w[0], w[1] = -1500.0, 1500.0
    return build(wfn(4, 7, 4), theta, lam, u, v, w, rng)


def screen_turns(c):
    """the largest phase of a case's screens, in turns: max |wc_l| x max ph over the cells inside the horizon"""
    N, theta, ref = c["N"], c["theta"], c["ref"]
    x = (np.arange(N, dtype=np.float64) - np.float64(N // 2)) / np.float64(N) * np.float64(theta)
    r2 = x[None, :] ** 2 + x[:, None] ** 2
    ph = 1.0 - np.sqrt(1.0 - r2[r2 < 1.0])
    wc = np.abs(ref.lay["pc"][ref.occupied].astype(np.float64) * ref.wstep)
    return float(wc.max() * ph.max())


def subgrid_turns(c):
    """the largest phase of an image-domain case's subgrid sums: (|a| + |b|) / 2 + |dw| x max ph over the pixels inside the
    horizon (|f| <= 1/2)"""
    ref = c["ref"]
    k = ref.keep
    return float(((np.abs(ref.a[k]) + np.abs(ref.b[k])) / 2 + np.abs(ref.dw[k]) * ref.ph[ref.ok].max()).max())


# ---- D: degenerate streams and the limit --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_visibility():
    rng = np.random.default_rng(500)
    return build(wfn(3, 7, 2), THETA48, LAM48, [37.0], [-51.0], [420.0], rng)


@functools.lru_cache(maxsize=None)
def no_finite_w():
    rng = np.random.default_rng(510)
    u, v = uv(rng, 5, LAM48)
    v[0], v[1] = -abs(v[0]), abs(v[1])  # (either side of do_imaging's mirror)
    return build(wfn(3, 7, 2), THETA48, LAM48, u, v, [np.nan, np.inf, -np.inf, np.nan, np.inf], rng)


TWO52 = 4503599627370496.0  # 2^52: with wstep = 1 the largest plane a stack takes


# ---- H: the horizon (image-domain layers) -------------------------------------------------------------------------------
HORIZON = {(16, 8): 32, (24, 12): 24, (32, 16): 33}  # (subgrid, margin) -> lam; theta = 2.0: N = 64, 48, 66
HORIZON_THETA, HORIZON_WSTEP = 2.0, 20


@functools.lru_cache(maxsize=None)
def horizon(sk):
    lam = HORIZON[sk]
    rng = np.random.default_rng(600 + sk[0])
    n = 300
    u, v = uv(rng, n, lam, 0.45)
    w = rng.uniform(-90.0, 90.0, n)
    w[0], w[1] = -90.0, 90.0  # the planes -5 and 5 (ties, at that): centre planes -3, 1 and 5, screens below 100 turns
    return build(ifn(sk, 4, HORIZON_WSTEP), HORIZON_THETA, lam, u, v, w, rng)


def beyond(c):
    """the image cells on and beyond the horizon, l^2 + m^2 >= 1 (wstack_ref.screen's rule)"""
    return W.screen(c["theta"], c["N"], 0.0) == 0.0


# ---- G: the degridder's widths (image-domain layers) --------------------------------------------------------------------
SUBGRIDS = ((16, 8), (24, 12), (32, 16))
WIDTH_N = (64, 65, 128, 129, 2 * SPLIT)
WIDTH_THETA, WIDTH_LAM = 0.1, 640  # N = 64, as test_gpu_idg.py
MIXED_N = {(16, 8): 64, (24, 12): 64, (32, 16): 96}  # (at N = 64 there are only 16 tiles of 16 cells)


def tile_uv(rng, sk, n, ty=None, tx=None, N=64):
    """n points in the tile (ty, tx) of T = Sg - K cells (default: the one that holds cell 24), the first on its corner;
    lam = 10 N, so that the corner's cell coordinate is exact"""
    T = sk[0] - sk[1]
    ty, tx = 24 // T if ty is None else ty, 24 // T if tx is None else tx
    x, y = rng.uniform(tx * T, (tx + 1) * T, n), rng.uniform(ty * T, (ty + 1) * T, n)
    x[0], y[0] = tx * T, ty * T
    return (x - N // 2) * 10.0, (y - N // 2) * 10.0


@functools.lru_cache(maxsize=None)
def width(sk, n):
    """one tile near the centre with n visibilities, all in one layer (test_one_tile_either_side_of_the_chunk_and_the_split
    of test_gpu_idg.py)"""
    rng = np.random.default_rng(700 + n)
    u, v = tile_uv(rng, sk, n)
    return build(ifn(sk, 4), WIDTH_THETA, WIDTH_LAM, u, v, rng.uniform(-40.0, 40.0, n), rng)


@functools.lru_cache(maxsize=None)
def mixed(sk):
    """one layer: a tile of SPLIT + 76 visibilities (a full work item of 1024 and one of 76) and 20 tiles of one each -
    22 items with a mean of 50, so the full item runs under the 64-thread launch"""
    rng = np.random.default_rng(710 + sk[0])
    T, N = sk[0] - sk[1], MIXED_N[sk]
    nt = N // T  # (the tiles that lie wholly on the grid)
    big = (24 // T, 24 // T)
    others = [(ty, tx) for ty in range(nt) for tx in range(nt) if (ty, tx) != big]
    pick = rng.choice(len(others), 20, replace=False)
    parts = [tile_uv(rng, sk, SPLIT + 76, N=N)] + [tile_uv(rng, sk, 1, *others[i], N=N) for i in pick]
    u, v = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    perm = rng.permutation(len(u))
    return build(ifn(sk, 4), WIDTH_THETA, 10 * N, u[perm], v[perm], rng.uniform(-40.0, 40.0, len(u)), rng)


def items(c):
    """(tiles, work items, visibilities) of every occupied layer of an image-domain case, as idg_partition cuts them"""
    ref = c["ref"]
    out = []
    for l in ref.occupied:
        counts = [len(idx) for _, _, idx in ref._items(l)]
        out.append((len(counts), sum(-(-k // SPLIT) for k in counts), sum(counts)))
    return out
