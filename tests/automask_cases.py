"""The inputs of the automask tests (tests/test_automask_host.py, tests/test_gpu_automask.py): small images built around
the labelling tile of csrc/automask.hip, whose size is read from the source.  A case is (name, image, mask0, keywords of
automask_ref.automask / Context.automask); every labelling case has hand-set floor levels (nsigma 0, no noise), so that
the sets H and L are exact."""
import os
import re

import numpy as np

from conftest import PKG


def tile():
    """(th, tw): the labelling tile of csrc/automask.hip"""
    src = open(os.path.join(PKG, "csrc", "automask.hip")).read()
    m = re.search(r"constexpr int AM_TH = (\d+), AM_TW = (\d+);", src)
    return int(m.group(1)), int(m.group(2))


def sizes():
    th, tw = tile()
    return [1, 2, 3, tw - 1, tw + 1, 2 * tw + 3]


FIXED = dict(nsigma=(0.0, 0.0), noise=None)


def patterns(N):
    """name -> boolean N x N set, the shapes a labelling can get wrong"""
    th, tw = tile()
    yy, xx = np.mgrid[0:N, 0:N]
    out = {"empty": np.zeros((N, N), dtype=bool), "all set": np.ones((N, N), dtype=bool)}
    c = np.zeros((N, N), dtype=bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    out["a cell in each corner"] = c
    out["checkerboard"] = (yy + xx) % 2 == 0  # one component under 8-connectivity, N * N / 2 under 4
    out["checkerboard, odd"] = (yy + xx) % 2 == 1
    if N > max(th, tw):  # two cells touching only diagonally across the corner where four tiles meet, both ways
        d = np.zeros((N, N), dtype=bool)
        d[th - 1, tw - 1] = d[th, tw] = True
        out["diagonal across four tiles"] = d
        d = np.zeros((N, N), dtype=bool)
        d[th - 1, tw] = d[th, tw - 1] = True
        out["anti-diagonal across four tiles"] = d
        e = np.zeros((N, N), dtype=bool)  # bars cut by each tile edge, and two that only come close
        e[th - 3:th + 3, 5] = e[7, tw - 3:tw + 3] = True
        if N > max(th + 1, tw + 5):
            e[th - 1, tw + 5] = e[th + 1, tw + 5] = True
        out["cut by each tile edge"] = e
    if N >= 3:
        u = np.zeros((N, N), dtype=bool)  # a U whose arms join only in the last row
        u[:, 0] = u[:, -1] = u[-1, :] = True
        out["U"] = u
        s = np.zeros((N, N), dtype=bool)  # one cell wide: every other row, joined at alternating ends
        s[0::4, :] = s[2::4, :] = True
        s[1::4, -1] = s[3::4, 0] = True
        out["serpentine"] = s
        n = np.zeros((N, N), dtype=bool)  # the same turned: every other column (a run per cell in every row)
        n[:, 0::4] = n[:, 2::4] = True
        n[-1, 1::4] = n[0, 3::4] = True
        out["serpentine, upright"] = n
    if N > 3:
        rng = np.random.default_rng(N)
        for p in (0.3, 0.45, 0.6):  # below, near and above the percolation of 8-connected sites
            out[f"random {p}"] = rng.random((N, N)) < p
    return out


def labelling_cases(N):
    """Each pattern three ways, so that what the labelling found shows in the mask and not only in the counts:
    as it is; pruned at the size of its largest component (kept only if the labelling joined all of it) and one more
    (nothing kept); and with one seed at its last cell above T_hi and the rest between the levels (hysteresis keeps the
    seed's whole component of L and nothing else)."""
    import automask_ref
    cases = []
    for name, inset in patterns(N).items():
        image = inset.astype(np.float64)
        zero = np.zeros((N, N), dtype=np.uint8)
        cases.append((name, image, zero, dict(thr=(0.5, 0.5), **FIXED)))
        lab = automask_ref.label(inset)
        if inset.any():
            big = int(np.unique(lab[lab >= 0], return_counts=True)[1].max())
            cases.append((name + ", pruned at the largest", image, zero, dict(thr=(0.5, 0.5), min_cells=big, **FIXED)))
            cases.append((name + ", pruned above it", image, zero, dict(thr=(0.5, 0.5), min_cells=big + 1, **FIXED)))
            seeded = image.copy()
            seeded.flat[np.flatnonzero(inset)[-1]] = 2.0
            cases.append((name + ", one seed", seeded, zero, dict(thr=(1.5, 0.5), **FIXED)))
    return cases


def feature_cases():
    """pruning, hysteresis, growing, accumulation, non-finite cells, absolute"""
    th, tw = tile()
    N = tw + 5
    cases = []
    zero = np.zeros((N, N), dtype=np.uint8)
    # a component of exactly min_cells cells is kept, one of min_cells - 1 dropped: a 2 x 3 block and an L of 5 cells
    img = np.zeros((N, N))
    img[2:4, 2:5] = 1.0
    img[10:13, 10] = img[12, 11:13] = 1.0
    cases.append(("six kept, five dropped", img, zero, dict(thr=(0.5, 0.5), min_cells=6, **FIXED)))
    # L components: one holding a surviving and a pruned H component (kept whole), one holding only a pruned one (dropped)
    img = np.zeros((N, N))
    img[5, 2:30] = 1.0
    img[5, 3:7] = 2.0       # survives min_cells = 3
    img[5, 20] = 2.0        # pruned, but in the same island of L
    img[20, 2:12] = 1.0
    img[20, 5:7] = 2.0      # pruned, alone in its island
    cases.append(("hysteresis", img, zero, dict(thr=(1.5, 0.5), min_cells=3, **FIXED)))
    # growing at the rim and with a border: nothing outside the region is set
    img = np.zeros((N, N))
    img[0, 0] = img[N - 1, N // 2] = img[N // 2, N - 1] = img[N // 2, N // 2] = 1.0
    for g in (0, 1, 32):
        cases.append((f"grow {g} at the rim", img, zero, dict(thr=(0.5, 0.5), grow=g, **FIXED)))
        cases.append((f"grow {g}, border 3", img, zero, dict(thr=(0.5, 0.5), grow=g, border=3, **FIXED)))
    # accumulation: bytes of 5 survive as 5, new cells are 1, nothing is cleared
    start = np.zeros((N, N), dtype=np.uint8)
    start[N // 2 - 1:N // 2 + 1, :] = 5
    start[3, 3] = 200
    cases.append(("accumulation", img, start, dict(thr=(0.5, 0.5), grow=2, **FIXED)))
    # NaN and +-Inf never take part, but may be grown over
    bad = img.copy()
    bad[N // 2, N // 2 + 1], bad[N // 2 + 1, N // 2], bad[N // 2 - 1, N // 2] = np.nan, np.inf, -np.inf
    bad[1, 1] = np.inf
    for absolute in (False, True):
        cases.append((f"non-finite cells, absolute {absolute}", bad, zero,
                      dict(thr=(0.5, 0.5), grow=1, absolute=absolute, **FIXED)))
    # a negative island: in the mask with absolute, not without; peak_frac picks the level from the peak
    neg = np.zeros((N, N))
    neg[4:7, 4:7] = -3.0
    neg[20:22, 20:22] = 2.0
    neg[30, 30] = 0.5
    for absolute in (False, True):
        cases.append((f"negative island, absolute {absolute}", neg, zero,
                      dict(thr=(1.0, 0.25), absolute=absolute, **FIXED)))
        cases.append((f"peak_frac, absolute {absolute}", neg, zero,
                      dict(thr=(0.0, 0.0), peak_frac=0.5, absolute=absolute, **FIXED)))
    # an all-negative image without absolute: peak_frac * P is negative and the floor 0 stands
    cases.append(("all negative", -np.abs(neg) - 1.0, zero, dict(thr=(0.0, 0.0), peak_frac=0.5, **FIXED)))
    # nothing takes part: reason 2, the mask untouched
    cases.append(("all NaN", np.full((N, N), np.nan), start, dict(thr=(0.5, 0.5), **FIXED)))
    return cases
