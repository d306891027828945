"""Inputs that test_aw_batches_host.py (host) and test_gpu_aw_batches.py (GPU) share: small aw streams whose structure
sits at the cuts of the batch loop of csrc/awgrid.hip (option "aw_batch"), and streams whose keys make the key cache's
hash table probe past its last slot.  No GPU: plain numpy.  The host test shows that every fixture has the property it
is named for, and computes the figures the GPU test demands of the library's counters.

The key of a visibility is (a1, a2, wbin, yf, xf); with the cache each batch builds one kernel per distinct key of its
kept visibilities, and a visibility is dropped (nothing gridded, an exact 0 predicted) when wbin, a1 or a2 is out of
range or u or v is NaN.  gridhip_last_dropped counts the first kind, as include/gridhip.h says of it and of awdegrid:
a NaN coordinate is off the grid, like a coordinate beyond its rim, and every gridder of the library drops those
without counting them (bin.hip's vis_bin looks at the coordinates first).  No fixture drops one visibility in both
ways, and every finite coordinate lies within +-0.4 of the grid, so nothing else is dropped."""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name N W Q S A wk ak u v wb a1 a2 vis B")

HASH_MUL = 0x9E3779B97F4A7C15
HSLOTS = 1024  # the smallest table: batches of up to 512 visibilities


def stream(seed, N, W, Q, S, A, nb, dumps, drift=0.02):
    """test_gpu_aw.py's _aw_case: nb baselines x `dumps` consecutive samples drifting by `drift` cells each"""
    rng = np.random.default_rng(seed)
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(A, S, S)) + 1j * rng.normal(size=(A, S, S))
    u0, v0 = rng.uniform(-0.4, 0.4, nb), rng.uniform(-0.4, 0.4, nb)
    ang = rng.uniform(0, 2 * np.pi, nb)
    d = np.arange(dumps)
    u = (u0[:, None] + d[None, :] * np.cos(ang)[:, None] * drift / N).ravel()
    v = (v0[:, None] + d[None, :] * np.sin(ang)[:, None] * drift / N).ravel()
    rep = lambda a: np.repeat(a, dumps)  # noqa: E731
    wb, a1, a2 = rep(rng.integers(0, W, nb)), rep(rng.integers(0, A, nb)), rep(rng.integers(0, A, nb))
    n = nb * dumps
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    return wk, ak, u, v, wb, a1, a2, vis


def _case(name, seed, N, W, Q, S, A, nb, dumps, B, drift=0.02):
    return Case(name, N, W, Q, S, A, *stream(seed, N, W, Q, S, A, nb, dumps, drift), B)


def _drop(c, k, how):
    """visibility k dropped in one of the six ways"""
    if how == 0:
        c.wb[k] = c.W
    elif how == 1:
        c.a1[k] = -1
    elif how == 2:
        c.a2[k] = c.A
    elif how == 3:
        c.u[k] = np.nan
    elif how == 4:
        c.wb[k] = -1
    else:
        c.v[k] = np.nan


def kept(c):
    return ((c.wb >= 0) & (c.wb < c.W) & (c.a1 >= 0) & (c.a1 < c.A) & (c.a2 >= 0) & (c.a2 < c.A) & ~np.isnan(c.u) &
            ~np.isnan(c.v))


def counted(c):
    """the dropped visibilities gridhip_last_dropped counts: an index out of range (at a finite coordinate)"""
    return ~kept(c) & ~np.isnan(c.u) & ~np.isnan(c.v)


def batches(c):
    n = len(c.u)
    return [(lo, min(lo + c.B, n)) for lo in range(0, n, c.B)]


def keys(c, frac_coord):
    """(n, 5) int64: (a1, a2, wbin, yf, xf) per visibility, rows of -1 for the dropped ones; frac_coord: the oracle's"""
    keep = kept(c)
    out = np.full((len(c.u), 5), -1, dtype=np.int64)
    _, xf = frac_coord(c.N, c.Q, c.u[keep])
    _, yf = frac_coord(c.N, c.Q, c.v[keep])
    out[keep] = np.stack([c.a1[keep], c.a2[keep], c.wb[keep], yf, xf], axis=1)
    return out


def figures(c, frac_coord):
    """what the library's counters must report: (distinct kept keys per batch, their sum, the counted drops, the
    distinct kept keys of the whole stream)"""
    k, keep = keys(c, frac_coord), kept(c)
    distinct = lambda rows: len({tuple(r) for r in rows})  # noqa: E731
    per = [distinct(k[lo:hi][keep[lo:hi]]) for lo, hi in batches(c)]
    return per, sum(per), int(counted(c).sum()), distinct(k[keep])


# ---- (a) structure at the cut ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cut_cases():
    out = []
    # n an exact multiple of B (240 = 4 x 60)
    out.append(_case("multiple", 101, 64, 2, 2, 5, 4, 40, 6, 60))
    # n = 3 x 100 + 1: the last batch holds one visibility
    out.append(_case("plus-one", 102, 80, 3, 2, 9, 5, 43, 7, 100))
    # one visibility per batch
    out.append(_case("one-each", 103, 64, 2, 2, 5, 4, 12, 5, 1))
    # every baseline's 8 dumps share one key (no drift); the cut at 100 = 12 x 8 + 4 lies inside baseline 12's run
    out.append(_case("straddle", 104, 96, 2, 2, 12, 4, 30, 8, 100, drift=0.0))
    # batch 2 = [96, 144) holds dropped visibilities only, in all six ways; a few more elsewhere
    c = _case("dropped-batch", 105, 72, 3, 2, 9, 5, 40, 6, 48)
    for k in range(96, 144):
        _drop(c, k, k % 6)
    for i, k in enumerate((0, 47, 48, 95, 144, 239)):  # the first and the last visibility of other batches
        _drop(c, k, i)
    out.append(c)
    # batch 1 = [60, 120) has the one pair (2, 1), which baseline 3 (batch 0) has too and no later batch has
    c = _case("old-pair", 106, 64, 2, 2, 12, 4, 30, 6, 60)
    swap = (c.a1 == 2) & (c.a2 == 1)
    c.a1[swap] = 1
    c.a1[60:120], c.a2[60:120] = 2, 1
    c.a1[18:24], c.a2[18:24] = 2, 1
    out.append(c)
    for c in out:
        for a in c[6:14]:
            a.setflags(write=False)
    return tuple(out)


# ---- (b) a probe that wraps -----------------------------------------------------------------------------------------
def home(key):
    """the slot aw_keys_kernel probes first in a table of 1024"""
    return (((int(key) * HASH_MUL) & 0xFFFFFFFFFFFFFFFF) >> 32) & (HSLOTS - 1)


def probe(keys_in_order):
    """linear probing into 1024 slots in the given insertion order -> {key: slot}"""
    tab, where = {}, {}
    for k in keys_in_order:
        h = home(k)
        while h in tab and tab[h] != k:
            h = (h + 1) & (HSLOTS - 1)
        tab[h] = k
        where[k] = h
    return where


WRAP_W, WRAP_Q, WRAP_S, WRAP_N = 64, 8, 5, 64  # 4096 slices of 5 x 5: a 1.6 MB table
TAIL = (1021, 1022, 1023)


def wrap_keys():
    """every slice whose home slot is one of the last three: with A = 2 and the one pair (0, 1) the pair slot is 0 and
    the key is the slice (wbin * Q + yf) * Q + xf itself"""
    return [k for k in range(WRAP_W * WRAP_Q * WRAP_Q) if home(k) in TAIL]


@functools.lru_cache(maxsize=None)
def wrap_cases():
    """480 visibilities, each half = the wrapping keys first, then keys found nowhere else; one batch of 480 (46 % load)
    and two of 240, the wrapping keys recurring in the second"""
    W, Q, S, N = WRAP_W, WRAP_Q, WRAP_S, WRAP_N
    rng = np.random.default_rng(107)
    chosen = wrap_keys()[:10]
    rest = [int(k) for k in rng.permutation(W * Q * Q) if home(int(k)) not in TAIL]
    half = 240 - len(chosen)
    sl = np.array(chosen + rest[:half] + chosen + rest[half:2 * half], dtype=np.int64)
    # the halves in random order each (the wrapping keys anywhere in their batch)
    sl = np.concatenate([rng.permutation(sl[:240]), rng.permutation(sl[240:])])
    n = len(sl)
    wb, yf, xf = sl // (Q * Q), (sl // Q) % Q, sl % Q
    # cell + f / Q is exact in binary, and so is the coordinate: frac_coord gives back (cell, f)
    cx, cy = rng.integers(8, N - 8, n), rng.integers(8, N - 8, n)
    u, v = (cx + xf / Q - N // 2) / N, (cy + yf / Q - N // 2) / N
    wk = rng.normal(size=(W, Q, Q, S, S)) + 1j * rng.normal(size=(W, Q, Q, S, S))
    ak = rng.normal(size=(2, S, S)) + 1j * rng.normal(size=(2, S, S))
    a1, a2 = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    vis = rng.normal(size=n) + 1j * rng.normal(size=n)
    for a in (wk, ak, u, v, wb, a1, a2, vis):
        a.setflags(write=False)
    return tuple(Case(name, N, W, Q, S, 2, wk, ak, u, v, wb, a1, a2, vis, B) for name, B in (("wrap-one", 512), ("wrap-two", 240)))


def slices_of(c, frac_coord):
    """the w-kernel slice of every visibility of a wrap case = its key"""
    k = keys(c, frac_coord)
    return (k[:, 2] * c.Q + k[:, 3]) * c.Q + k[:, 4]


def all_cases():
    return cut_cases() + wrap_cases()


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ---- what the GPU test compares with --------------------------------------------------------------------------------
def for_the_restatement(c):
    """(u, v, wb) in which every dropped visibility is dropped by wbin = -1 at a finite coordinate: the numpy
    restatement of the gather looks at the indices only"""
    keep = kept(c)
    return np.where(keep, c.u, 0.0), np.where(keep, c.v, 0.0), np.where(keep, c.wb, -1)


def imaging_form(c, theta=0.008):
    """The stream as the imaging interface takes it: (lam, wvals, uvw in wavelengths) with N = theta * lam and
    findClosest(wvals, w) = wbin.  That interface cannot give a w-bin outside the table."""
    assert ((c.wb >= 0) & (c.wb < c.W)).all() and not np.isnan(c.u).any()
    lam = int(round(c.N / theta))
    assert int(np.rint(theta * lam)) == c.N
    wvals = np.linspace(-100.0, 100.0, c.W)
    return lam, wvals, (c.u * lam, c.v * lam, wvals[c.wb])
