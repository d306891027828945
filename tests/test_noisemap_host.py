"""CPU checks of the local background and noise maps: the numpy restatement (tests/noisemap_ref.py) against a brute-force
sort of every window and against hand-computed cells, the mesh the library reports against the restatement's, and the
effect the maps exist for, kept on record."""
import math

import numpy as np
import pytest

import noise_ref
import noisemap_ref as ref


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- the node statistic ---------------------------------------------------------------------------------------------------
def brute_window(v, kappa, nclip):
    """np.sort of the values themselves (no keys), round by round"""
    r = 0
    while True:
        s = np.sort(v)
        med = s[(s.size - 1) // 2]
        d = np.abs(v - med)
        mad = np.sort(d)[(d.size - 1) // 2]
        if r == nclip or not (d > kappa * (1.4826 * mad)).any():
            return med, mad, v.size, r
        v = v[d <= kappa * (1.4826 * mad)]
        r += 1


@pytest.mark.parametrize("nclip", [0, 1, 3, 8])
@pytest.mark.parametrize("N, border, step, half", [(37, 3, 5, 4), (40, 0, 16, 9), (7, 0, 16, 3), (1, 0, 1, 1)])
def test_node_table_is_a_sort_of_each_window(N, border, step, half, nclip):
    rng = np.random.default_rng(N + nclip)
    img = rng.normal(size=(N, N))
    img[rng.random((N, N)) < 0.05] += 40.0  # outliers for the clip rounds to drop
    if N > 4:
        img[2 % N, 3 % N] = np.nan
    mask = rng.random((N, N)) < 0.8
    for exclude in (False, True):
        nodes = ref.node_table(img, mask, exclude, border, step, half, 2.5, nclip, 5)
        c = ref.centres(N, border, step)
        assert nodes.shape == (4, len(c), len(c))
        for i, cy in enumerate(c):
            for j, cx in enumerate(c):
                cells = [img[y, x] for y in range(max(border, cy - half), min(N - border, cy + half + 1))
                         for x in range(max(border, cx - half), min(N - border, cx + half + 1))
                         if np.isfinite(img[y, x]) and bool(mask[y, x]) != exclude]
                if not cells:
                    want = (math.nan, math.nan, 0.0, 0.0)
                else:
                    med, mad, n, r = brute_window(np.array(cells), 2.5, nclip)
                    want = (med if n >= 5 else math.nan, 1.4826 * mad if n >= 5 and mad > 0 else math.nan, float(n), float(r))
                assert same(nodes[:, i, j], np.array(want)), (i, j, nodes[:, i, j], want)
    if nclip >= 1 and N > 30:
        assert nodes[3].max() >= 1, "no window dropped an outlier: the clip rounds are not exercised"


def test_clip_stops_at_a_tie_with_the_limit():
    """d_k == L stays (the test is d_k > L): three values 0, 1, 2 around the median 1 with kappa = 1 / 1.4826 ..."""
    v = np.array([0.0] * 3 + [1.0] * 5 + [2.0] * 3 + [9.0])
    kappa = 1.0 / 1.4826
    L = kappa * (1.4826 * 1.0)
    med, mad, n, r = ref.node_stat(v, kappa, 3)
    assert (med, mad) == (1.0, 1.0)
    assert n == int(np.count_nonzero(np.abs(v - 1.0) <= L)) and r == 1


# ---- the mesh and the interpolation ---------------------------------------------------------------------------------------
def test_centres():
    assert ref.centres(16, 2, 4) == [4, 8, 12]
    assert ref.centres(7, 0, 16) == [6]  # M < step: one node, its centre clamped to M - 1
    assert ref.centres(1, 0, 1) == [0]
    assert ref.centres(37, 3, 5) == [5, 10, 15, 20, 25, 30]
    assert ref.centres(130, 0, 1) == list(range(130))


def test_interpolation_hand_computed():
    N, border, step = 16, 2, 4  # centres 4, 8, 12
    t = np.array([[10.0 * i + j for j in range(3)] for i in range(3)])
    c = ref.centres(N, border, step)
    assert ref.locate(3, c) == (0, 1, 0.0) and ref.locate(4, c) == (0, 1, 0.0) and ref.locate(5, c) == (0, 1, 0.25)
    assert ref.locate(12, c) == (2, 2, 0.0) and ref.locate(13, c) == (2, 2, 0.0)
    assert ref.interp_cell(t, c, 2, 3) == 0.0  # before c_0 on both axes: t[0][0]
    assert ref.interp_cell(t, c, 3, 10) == 1.5  # before c_0 in y, half way between nodes 1 and 2 in x
    assert ref.interp_cell(t, c, 5, 10) == 4.0  # top 1.5, bottom 11.5, a quarter of the way down
    assert ref.interp_cell(t, c, 13, 13) == 22.0  # after the last centre: t[2][2]
    assert ref.interp_cell(t, c, 13, 6) == 20.5
    # the fallbacks: only a finite, only b finite, neither
    nan = math.nan
    assert ref.lerp(1.0, nan, 0.25) == 1.0 and ref.lerp(nan, 2.0, 0.25) == 2.0 and math.isnan(ref.lerp(nan, math.inf, 0.5))
    t[0, 1] = t[0, 2] = t[2, 0] = nan
    assert ref.interp_cell(t, c, 4, 6) == 0.0    # top: only a (t[0][0]); bottom 10.5; fy = 0
    assert ref.interp_cell(t, c, 4, 10) == 11.5  # top: neither; the outer lerp then has only b, the bottom 11.5
    assert ref.interp_cell(t, c, 6, 8) == 11.0   # the same half way down
    assert ref.interp_cell(t, c, 12, 6) == 21.0  # both rows are node 2: only b (t[2][1]) twice, then 21 + 0 * 0
    assert ref.interp_cell(t, c, 2, 10) == 11.5  # before c_0 in y, fy = 0: the fallback to the bottom row holds all the same
    # the whole-image form is the per-cell form, bit for bit, and NaN outside the border region
    m = ref.interp_map(t, N, border, step)
    for y in range(N):
        for x in range(N):
            if border <= y < N - border and border <= x < N - border:
                assert same(np.array(m[y, x]), np.array(ref.interp_cell(t, c, y, x))), (y, x)
            else:
                assert math.isnan(m[y, x])


def test_library_mesh_is_the_restatement():
    """gridhip_noise_map_nodes and gridhip.noise_grid need no device"""
    import gridhip
    from gridhip import _lib
    lib = _lib.load()
    for N, border, step in [(1, 0, 1), (7, 0, 16), (37, 3, 5), (150, 0, 40), (130, 0, 1), (257, 0, 16), (2400, 10, 32)]:
        c = ref.centres(N, border, step)
        assert lib.gridhip_noise_map_nodes(N, border, step) == len(c)
        got = gridhip.noise_grid(N, border, step)
        assert got.dtype == np.int64 and got.tolist() == c
    for bad in [(0, 0, 1), (8, -1, 1), (8, 4, 1), (8, 0, 0)]:
        assert lib.gridhip_noise_map_nodes(*bad) == _lib.EINVAL
        with pytest.raises(gridhip.GridHipError):
            gridhip.noise_grid(*bad)


# ---- the effect, on record --------------------------------------------------------------------------------------------------
def ramp_image(seed, N=192):
    """sigma ramping from 1 to 4 across the field, offset 0.5, one 200-unit Gaussian source (sigma 3 cells) at the centre"""
    rng = np.random.default_rng(seed)
    sigma = np.broadcast_to(np.linspace(1.0, 4.0, N)[None, :], (N, N))
    y, x = np.mgrid[0:N, 0:N]
    r2 = (y - N // 2) ** 2 + (x - N // 2) ** 2
    img = 0.5 + sigma * rng.normal(size=(N, N)) + 200.0 * np.exp(-r2 / (2.0 * 3.0 ** 2))
    return img, sigma, r2 > 16 ** 2  # the last: the cells outside the source (it is below 1e-4 there)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_local_noise_against_a_global_level(seed):
    """N = 192, step 16, half 16, three clip rounds.  Measured with this restatement, seeds 0, 1, 2: noise cells above
    4 sigma outside the source 57, 82, 55 with the global level median + 4 * 1.4826 * MAD and 4, 4, 0 with the local S/N
    image (the Gaussian expectation is about 1.2); median relative error of the rms map against the true sigma 0.022,
    0.032, 0.026.  (The source here has a sigma of 3 cells and "outside" is more than 16 cells from it.)"""
    img, sigma, outside = ramp_image(seed)
    _, rms, snr, _, stats = ref.noise_map(img, step=16, half=16, nclip=3, mode="snr")
    g = noise_ref.image_stats(img)
    n_global = int(np.count_nonzero((img > g[1] + 4.0 * g[3]) & outside))
    n_local = int(np.count_nonzero((snr > 4.0) & outside))
    err = float(np.median(np.abs(rms - sigma) / sigma))
    print(f"seed {seed}: global {n_global}, local {n_local}, median relative rms error {err:.4f}")
    assert stats[1] == stats[2] == 144 and stats[5] == 0
    assert err < 0.05
    assert n_global >= 5 * n_local and n_global > 0
