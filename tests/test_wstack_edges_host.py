"""The preconditions of tests/wstack_edge_cases.py, on the restatements alone: no GPU.  Every case is shown to reach the
edge it is named after, so that test_gpu_wstack_edges.py pins the device there and not somewhere near it.

- T: every w of the tie stream is an exact tie or the double next to one; the plane rule gives pmin = -7, and a half-even
  rule gives pmin = -6 and another image, for every M.
- S: more visibilities than one work-group of the scatter ranks where claimed, and every layer occupied.
- C: more layers than the scan has threads, the layers and the occupied ones as stated.
- F: finite tables and outputs, no horizon, screens of at least 500 turns.
- H: subgrid pixels and trusted image cells beyond the horizon, two pixels exactly on it, phases below 100 turns.
- G: one layer, the tiles and work items as stated, the layer's mean item on the intended side of 64 and 128."""
import numpy as np
import pytest

import idg_ref as I
import wstack_edge_cases as E
import wstack_ref as W


def finite(c):
    return bool(np.isfinite(c["image"]).all() and np.isfinite(c["pred"]).all())


# ---- T --------------------------------------------------------------------------------------------------------------------
def test_the_tie_stream_is_made_of_ties():
    w = E.tie_w()
    q = w / np.float64(E.WSTEP)
    assert len(w) == 14 * 12 + 4
    assert np.array_equal(q[:-4], np.repeat(np.arange(-7, 7), 12) + 0.5)  # exact halves
    assert np.array_equal(np.abs(q[-4:]), [np.nextafter(0.5, 0.0), np.nextafter(2.5, 0.0)] * 2)  # the doubles below a tie
    lay = W.layers(w, E.WSTEP, 1)
    p = lay["layer"] + lay["pmin"]
    assert np.array_equal(p[:-4], np.repeat(np.arange(-7, 7), 12) + (np.repeat(np.arange(-7, 7), 12) >= 0))  # away from 0
    assert p[-4:].tolist() == [0, 2, 0, -2]
    assert np.floor(q[-4] + 0.5) == 1.0  # (what adding a half and truncating would make of the first: q + 1/2 rounds to 1)


@pytest.mark.parametrize("M", [1, 2, 3])
def test_ties_tell_the_plane_rules_apart(M):
    c = E.ties(M)
    ref = c["ref"]
    assert ref.lay["pmin"] == -7 and ref.lay["L"] == 14 // M + 1 and finite(c)
    if M == 1:
        assert ref.lay["L"] == 15 and len(ref.occupied) == 15
    # ties straddle layer boundaries: a tie's two neighbouring planes lie in different layers
    lo = np.floor(c["w"] / E.WSTEP).astype(np.int64) - ref.lay["pmin"]
    assert M == 1 or np.any((lo // M != (lo + 1) // M) & (lo >= 0))
    with E.half_even():
        o = c["fn"][1]
        other = W.Stack(c["theta"], c["lam"], c["u"], c["v"], c["w"], o["wstep"], M, o["qpx"], o["npixFF"], o["npixKern"])
        assert other.lay["pmin"] == -6
        gap = np.abs(other.image(c["vis"]) - c["image"]).max() / np.abs(c["image"]).max()
        gap_p = np.abs(other.predict(c["model"]) - c["pred"]).max() / np.abs(c["pred"]).max()
    print(f"M={M}: half-even image {gap:.3g}, prediction {gap_p:.3g} of the maximum away")
    assert gap >= 1e-3 and gap_p >= 1e-3
    assert W.layers(c["w"], E.WSTEP, M)["pmin"] == -7  # (the rule is the restatement's own again)


def test_ties_through_image_domain_layers():
    c = E.ties_idg()
    ref = c["ref"]
    assert ref.lay["pmin"] == -7 and ref.lay["L"] == 8 and ref.dropped == 0 and finite(c)
    with E.half_even():
        other = I.Stack(c["theta"], c["lam"], c["u"], c["v"], c["w"], E.WSTEP, 2, 16, 8)
        assert other.lay["pmin"] == -6
        gap = np.abs(other.image(c["vis"]) - c["image"]).max() / np.abs(c["image"]).max()
    # (with exact residual w the image hardly depends on the plane; the partition does: pmin, and who is in which layer)
    print(f"idg: half-even image {gap:.3g} of the maximum away")
    assert not np.array_equal(other.lay["layer"], ref.lay["layer"])
    assert E.subgrid_turns(c) < 100 and E.screen_turns(c) < 100


# ---- S --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msq", E.SEAM_MSQ, ids=str)
@pytest.mark.parametrize("n", E.SEAM_N)
def test_scatter_seams(n, msq):
    c = E.seam(n, msq)
    groups = -(-n // E.SCATTER)
    assert groups == {2047: 1, 2048: 1, 2049: 2, 6145: 4}[n]
    assert c["n"] == n and c["ref"].lay["L"] == 9 and c["ref"].occupied == list(range(9)) and finite(c)


def test_scatter_seams_one_plane_and_every_layer():
    c = E.one_plane()
    assert -(-c["n"] // E.SCATTER) == 3 and c["ref"].lay["L"] == 1 and c["ref"].lay["pmin"] == 3
    c = E.every_layer()
    lay = c["ref"].lay
    assert -(-c["n"] // E.SCATTER) == 4 and lay["L"] == 16
    for g in range(4):  # every chunk of 2048 touches every layer
        assert set(lay["layer"][g * E.SCATTER:(g + 1) * E.SCATTER].tolist()) == set(range(16)) or g == 3
    assert len(set(lay["layer"][:3 * E.SCATTER].tolist())) == 16 and finite(c)
    N, msq, L, n = E.IMAGER_SEAM
    assert -(-n // E.SCATTER) > 1


# ---- C --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [257, 515])
def test_scan_seams(L):
    c = E.scan(L)
    ref = c["ref"]
    per = -(-L // E.SCAN)
    assert per == {257: 2, 515: 3}[L] and L % per != 0  # an odd tail: the last busy thread has fewer layers
    assert c["n"] == 2 * L + 3 and ref.lay["L"] == L and ref.occupied == E.scan_occupied(L) and finite(c)
    if L == 515:
        empty = sorted(set(range(L)) - set(ref.occupied))
        assert empty == list(range(1, L - 1, 3)) and len(empty) == 171


# ---- F --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [48, 65])
def test_wide_fields(N):
    c = E.wide(N)
    assert c["N"] == N and c["theta"] ** 2 / 2 < 1  # the image's corner lies inside the horizon
    assert not E.beyond(c).any()
    assert np.isfinite(c["ref"].K).all() and finite(c)
    turns = E.screen_turns(c)
    print(f"N={N}: screens up to {turns:.0f} turns")
    assert turns >= 500 and np.abs(c["w"]).max() <= 1500


# ---- D --------------------------------------------------------------------------------------------------------------------
def test_degenerate_streams():
    c = E.one_visibility()
    assert c["n"] == 1 and c["ref"].lay["L"] == 1 and finite(c) and np.abs(c["image"]).max() > 0
    c = E.no_finite_w()
    assert c["n"] == 5 and c["ref"].lay["L"] == 0 and c["dropped"] == 5 and c["ref"].occupied == []
    assert not c["image"].any() and not c["pred"].any() and (c["v"] < 0).any() and (c["v"] > 0).any()
    assert E.TWO52 == 2.0 ** 52 and E.TWO52 + 2 == float(2 ** 52 + 2)  # (both are doubles)
    assert W.layers(np.full(7, E.TWO52), 1, 1)["pmin"] == 2 ** 52


# ---- H --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sk,N,pixels,cells", [((16, 8), 64, 63, 24), ((24, 12), 48, 139, 24), ((32, 16), 66, 231, 12)], ids=str)
def test_horizon(sk, N, pixels, cells):
    c = E.horizon(sk)
    ref = c["ref"]
    assert c["N"] == N and ref.dropped == 0 and finite(c)
    assert int((~ref.ok).sum()) == pixels
    l = ref.f * np.float64(c["theta"])
    r2 = l[None, :] * l[None, :] + l[:, None] * l[:, None]
    on = np.argwhere(r2 == 1.0)
    assert sorted(map(tuple, on.tolist())) == [(0, sk[0] // 2), (sk[0] // 2, 0)]  # f = -1/2 on one axis, 0 on the other
    tr = I.trusted(N)
    out = E.beyond(c)
    assert int(out[tr, tr].sum()) == cells and out.sum() > cells
    assert not c["image"][out].any()
    a, b = E.screen_turns(c), E.subgrid_turns(c)
    print(f"{sk}: screens {a:.1f} turns, subgrid sums {b:.1f} turns")
    assert a < 100 and b < 100


# ---- G --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sk", E.SUBGRIDS, ids=str)
def test_degridder_widths(sk):
    want = {64: 64, 65: 128, 128: 128, 129: 256, 2 * E.SPLIT: 256}
    for n in E.WIDTH_N:
        c = E.width(sk, n)
        (tiles, nitems, nvis), = E.items(c)
        assert (tiles, nitems, nvis) == (1, -(-n // E.SPLIT), n) and c["ref"].dropped == 0 and finite(c)
        assert E.degrid_threads(nvis // nitems) == want[n]
        assert E.subgrid_turns(c) < 100 and E.screen_turns(c) < 100
    c = E.mixed(sk)
    assert c["N"] == E.MIXED_N[sk]
    (tiles, nitems, nvis), = E.items(c)
    assert (tiles, nitems, nvis) == (21, 22, E.SPLIT + 96) and c["ref"].dropped == 0 and finite(c)
    assert nvis // nitems < 64 and E.degrid_threads(nvis // nitems) == 64
    sizes = sorted(len(idx) for _, _, idx in c["ref"]._items(c["ref"].occupied[0]))
    assert sizes == [1] * 20 + [E.SPLIT + 76]
