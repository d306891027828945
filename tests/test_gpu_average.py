"""Phase shift and averaging on the device (gridhip_phase_shift[_dev], gridhip_average[_dev]) against the numpy restatement
tests/average_ref.py.  The shifted visibilities are compared to 1e-10 |vis| at |p| <= 1e4 turns - the DFT section's
derivation, three roundings of p cost 2 pi 3 1e4 2^-53 ~ 2e-11 - against a long-double reference; the shifted coordinates and
EVERYTHING the averaging writes are compared bit for bit (a generated NaN's sign aside): the sums are integer sums, so
there is no tolerance to state.  The shapes are the smallest at which each path can go wrong: a wave's and a work-group's
tails, groups whose neighbours share them (the run reduction) and do not, every n_g at which L changes, and one stream
long enough for a thread to take several visibilities."""
import ctypes as C

import numpy as np
import pytest

import average_ref as A
import dft_ref
from test_gpu_imager import host, to_dev

pytestmark = pytest.mark.gpu

c128, f64, i64 = np.complex128, np.float64, np.int64
SIZES = [1, 63, 64, 65, 255, 256, 257]
EINVAL, EUNSUPPORTED = -1, -5


def dev(x):
    return None if x is None else to_dev(x)


def rot(l0=0.04, m0=-0.03):
    import gridhip
    return gridhip.rotation_to(l0, m0)


def coords(rng, n, scale=1e5):
    """|p| <= 1e4 turns for centres up to 0.05 off axis"""
    return rng.uniform(-scale, scale, (3, n))


def noise(rng, n):
    return rng.normal(size=n) + 1j * rng.normal(size=n)


# ---- phase shift ------------------------------------------------------------------------------------------------------------
def check_shift(what, got, want, vis):
    out, uvw = got
    ref, (u1, v1, w1), _ = want
    err = np.abs(out - ref)
    lim = A.TOL * np.abs(vis)
    print(f"{what}: worst |vis' - ref| / |vis| {np.max(err[lim > 0] / np.abs(vis)[lim > 0], initial=0.0):.3e}")
    assert (err <= lim).all(), what
    if uvw is not None:
        assert A.same_bits(uvw[:, 0], u1) and A.same_bits(uvw[:, 1], v1) and A.same_bits(uvw[:, 2], w1), f"{what}: coordinates"


@pytest.mark.parametrize("n", SIZES)
def test_phase_shift_against_the_reference(ctx, n):
    rng = np.random.default_rng(n)
    R = rot()
    u, v, w = coords(rng, n)
    vis = noise(rng, n) * 10.0 ** rng.integers(-3, 4, n)
    want = A.phase_shift(R, u, v, w, vis)
    m = np.stack([u, v, w], axis=1)  # strided: an (n, 3) array
    for form, cv in (("host", np.asarray), ("dev", dev)):
        out, uvw = ctx.phase_shift(cv(m), cv(vis), R)
        check_shift(f"n {n} strided [{form}]", (np.asarray(host(out) if form == "dev" else out),
                                                np.asarray(host(uvw) if form == "dev" else uvw)), want, vis)
    out, uvw = ctx.phase_shift((dev(u), dev(v), dev(w)), dev(vis), R)
    check_shift(f"n {n} tuple", (host(out), host(uvw)), want, vis)
    dv = dev(vis)
    out = ctx.phase_shift(dev(m), dv, R, coords=False, out=dv)  # in place, no coordinates
    assert out is dv
    check_shift(f"n {n} in place", (host(dv), None), want, vis)
    hv = vis.copy()
    assert ctx.phase_shift(m, hv, R, coords=False, out=hv) is hv
    check_shift(f"n {n} in place [host]", (hv, None), want, vis)
    # w = None is w = 0
    want0 = A.phase_shift(R, u, v, None, vis)
    out, uvw = ctx.phase_shift((dev(u), dev(v), None), dev(vis), R)
    check_shift(f"n {n} no w", (host(out), host(uvw)), want0, vis)


def raw(ctx, name, *args):
    """the _dev entry point itself, on torch tensors: -> the return code"""
    from gridhip._marshal import device
    be = device()
    be.bind(ctx)
    args = [C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a for a in args]
    return getattr(ctx._lib, "gridhip_" + name + "_dev")(ctx._h, *args)


def Rptr(R):
    R = np.ascontiguousarray(R, dtype=f64)
    return R.ctypes.data_as(C.POINTER(C.c_double)), R


def test_phase_shift_of_coordinates_in_place_and_a_nan_coordinate(ctx):
    import torch
    rng = np.random.default_rng(7)
    n, R = 300, rot(-0.02, 0.05)
    u, v, w = coords(rng, n)
    u[5], w[77], v[299] = np.nan, np.inf, -np.inf
    vis = noise(rng, n)
    want = A.phase_shift(R, u, v, w, vis)
    assert want[2] == 3
    out, uvw, st = ctx.phase_shift(dev(np.stack([u, v, w], axis=1)), dev(vis), R, stats=True)
    check_shift("nan coordinate", (host(out), host(uvw)), want, vis)
    assert host(out)[[5, 77, 299]].tolist() == vis[[5, 77, 299]].tolist()  # passed through unchanged
    assert host(st).tolist() == [n - 3, 3, 0, 0]
    out, uvw, st = ctx.phase_shift(np.stack([u, v, w], axis=1), vis, R, stats=True)
    check_shift("nan coordinate [host]", (out, uvw), want, vis)
    assert st.tolist() == [n - 3, 3, 0, 0]
    # u_out == u, v_out == v, w_out == w (the columns of one interleaved array) and vis_out == vis_in
    m, dv = dev(np.stack([u, v, w], axis=1)), dev(vis)
    p, keep = Rptr(R)
    assert raw(ctx, "phase_shift", n, p, m[:, 0], m[:, 1], m[:, 2], 3, dv, dv, m[:, 0], m[:, 1], m[:, 2], 3, None) == 0
    torch.cuda.synchronize()
    check_shift("all in place", (host(dv), host(m)), want, vis)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 257])  # none, one, one work-group and one
def test_phase_shift_host_and_device_forms_give_the_same_bits(ctx, n, stride):
    """Every staging branch of gridhip_phase_shift: w, the coordinate outputs and stats present and null, the outputs at
    stride 1 and 3, vis and the coordinates out of place and in place.  One rounded sequence per visibility: the two forms
    give the same bits, and both agree with the reference as in the tests above."""
    rng = np.random.default_rng(500 + 10 * n + stride)
    R = np.ascontiguousarray(rot(0.03, -0.02), dtype=f64)
    u, v, w = coords(rng, n)
    vis = noise(rng, n)
    Rp = R.ctypes.data_as(C.POINTER(C.c_double))
    for with_w in (True, False):
        want = A.phase_shift(R, u, v, w if with_w else None, vis)
        for outs in ("none", "new", "in place"):
            for in_place in (False, True):
                for with_stats in (True, False):
                    # the three columns in one array: interleaved (stride 3) or one after the other (stride 1)
                    m = np.stack([u, v, w], axis=1 if stride == 3 else 0)
                    flat, off = m.reshape(-1).copy(), [0, 1, 2] if stride == 3 else [0, n, 2 * n]
                    vin = vis.copy()
                    vout = vin if in_place else np.full(n, 7 - 7j)
                    os_ = stride if outs == "in place" else 3
                    o = None if outs == "none" else flat if outs == "in place" else np.full(3 * max(n, 1), 7.0)
                    ooff = off if outs == "in place" else [0, 1, 2]
                    st = np.full(4, 7.0) if with_stats else None
                    hst, dvc = _shift_both(ctx, n, Rp, flat, off, with_w, stride, vin, vout, o, ooff, os_, st)
                    what = (n, stride, with_w, outs, in_place, with_stats)
                    for k in hst:
                        assert hst[k].tobytes() == dvc[k].tobytes(), what
                    uvw = None
                    if o is not None:
                        got = hst[id(o)]
                        uvw = np.stack([got[ooff[j]:ooff[j] + (n - 1) * os_ + 1:os_] if n else got[:0] for j in range(3)], axis=1)
                    check_shift(str(what), (hst[id(vout)], uvw), want, vis)
                    if st is not None:
                        assert hst[id(st)].tolist() == [n, 0, 0, 0], what


def _shift_both(ctx, n, Rp, flat, off, with_w, stride, vin, vout, o, ooff, os_, st):
    """gridhip_phase_shift and its _dev form on pointers into `flat` (and into `o`) at the given offsets in doubles"""
    import torch
    from gridhip._marshal import device
    lib, h = ctx._lib, ctx._h
    arrays = {id(a): a for a in (flat, vin, vout, o, st) if a is not None}
    hst = {k: a.copy() for k, a in arrays.items()}
    dvc = {k: to_dev(a if a.size else np.zeros(4, a.dtype)) for k, a in arrays.items()}  # (an empty tensor has no address)
    for base, ptr in ((hst, lambda a: a.ctypes.data), (dvc, lambda t: t.data_ptr())):
        at = lambda a, k=0: None if a is None else C.c_void_p(ptr(base[id(a)]) + 8 * k)  # noqa: E731
        args = [n, Rp, at(flat, off[0]), at(flat, off[1]), at(flat, off[2]) if with_w else None, stride, at(vin), at(vout),
                at(o, ooff[0]), at(o, ooff[1]), at(o, ooff[2]), os_, at(st)]
        if base is hst:
            assert lib.gridhip_phase_shift(h, *args) == 0
        else:
            device().bind(ctx)
            assert lib.gridhip_phase_shift_dev(h, *args) == 0
            torch.cuda.synchronize()
    return hst, {k: host(t)[:arrays[k].size] for k, t in dvc.items()}


def test_refusals(ctx):
    """every rule of the header that needs a context; nothing is touched by a refused call"""
    import torch
    import gridhip
    rng = np.random.default_rng(8)
    n, G = 16, 3
    m, vis = dev(rng.normal(size=(n, 3))), dev(noise(rng, n))
    grp = dev(rng.integers(0, G, n))
    m0, vis0 = host(m).copy(), host(vis).copy()
    bad_R = [np.eye(3) * 1.001, np.diag([1.0, -1.0, -1.0]), np.full((3, 3), np.nan), np.array([[1, 0, 0], [0, 1, 1e-8], [0, 0, 1.0]]),
             np.array([[0, 0, 1], [0, 1, 0], [-1.0, 0, 0]])]  # scaled; R22 < 0; NaN; sheared; R22 == 0
    for R in bad_R:
        with pytest.raises(gridhip.GridHipError) as e:
            ctx.phase_shift(m, vis, R)
        assert e.value.code == EINVAL
        with pytest.raises(gridhip.GridHipError) as e:
            ctx.average(m, vis, grp, G, R=R)
        assert e.value.code == EINVAL
    ctx.phase_shift(m, vis, np.eye(3) + 1e-11)  # within 1e-9 of a rotation
    p, keep = Rptr(np.eye(3))
    o3, ov, ow = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros_like(vis), torch.zeros(n, dtype=torch.float64, device="cuda")
    c, oc = (m[:, 0], m[:, 1], m[:, 2]), (o3[:, 0], o3[:, 1], o3[:, 2])
    shift = lambda *a: raw(ctx, "phase_shift", *a)  # noqa: E731
    assert shift(n, p, *c, 3, vis, ov, *oc, 3, None) == 0
    assert shift(n, None, *c, 3, vis, ov, *oc, 3, None) == EINVAL                  # no R
    assert shift(-1, p, *c, 3, vis, ov, *oc, 3, None) == EINVAL
    assert shift(n, p, None, c[1], c[2], 3, vis, ov, *oc, 3, None) == EINVAL       # no u
    assert shift(n, p, *c, 0, vis, ov, *oc, 3, None) == EINVAL                     # stride
    assert shift(n, p, *c, 3, vis, ov, *oc, 0, None) == EINVAL
    assert shift(n, p, *c, 3, vis, ov, oc[0], None, oc[2], 3, None) == EINVAL      # two of three coordinate outputs
    assert shift(n, p, *c, 3, vis, ov, c[1], c[0], c[2], 3, None) == EINVAL        # u_out is v
    assert shift(n, p, *c, 3, vis, ov, *c, 1, None) == EINVAL                      # in place at another stride
    assert shift(n, p, *c, 3, vis, m, *oc, 3, None) == EINVAL                      # vis_out over the coordinates
    assert shift(n, p, *c, 3, vis, ov, oc[0], oc[0], oc[2], 3, None) == EINVAL     # two outputs share elements
    assert shift(n, p, *c, 3, vis, ov, *oc, 3, ov) == EINVAL                       # stats over an output
    assert shift((1 << 31) - 256, p, *c, 3, vis, ov, *oc, 3, None) == EUNSUPPORTED
    assert shift(0, p, *c, 3, vis, ov, *oc, 3, None) == 0
    og, ovg, owg, ocg = (torch.zeros((G, 3), dtype=torch.float64, device="cuda"), torch.zeros(G, dtype=torch.complex128, device="cuda"),
                         torch.zeros(G, dtype=torch.float64, device="cuda"), torch.zeros(G, dtype=torch.int64, device="cuda"))
    g3 = (og[:, 0], og[:, 1], og[:, 2])
    avg = lambda *a: raw(ctx, "average", *a)  # noqa: E731
    good = lambda: [n, G, grp, None, *c, 3, None, vis, None, *g3, 3, None, ovg, owg, ocg, None]  # noqa: E731
    assert avg(*good()) == 0
    for i, val in ((0, -1), (1, 0), (2, None), (4, None), (7, 0), (9, None), (11, None), (14, 0), (16, None), (17, None)):
        a = good()
        a[i] = val
        assert avg(*a) == EINVAL, i
    a = good()
    a[8] = ow                                                                       # x without x_out
    assert avg(*a) == EINVAL
    a = good()
    a[16] = vis                                                                     # vis_out over vis
    assert avg(*a) == EINVAL
    a = good()
    a[17] = og[:, 0]                                                                # wt_out over u_out
    assert avg(*a) == EINVAL
    a = good()
    a[0] = (1 << 31) - 256
    assert avg(*a) == EUNSUPPORTED
    a = good()
    a[1] = (1 << 31) - 255
    assert avg(*a) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert np.array_equal(host(m), m0) and np.array_equal(host(vis), vis0)


# ---- physics -----------------------------------------------------------------------------------------------------------------
def test_a_point_at_the_new_centre_becomes_its_flux(ctx):
    import gridhip
    rng = np.random.default_rng(9)
    n, l0, m0, S = 500, 0.031, -0.027, 2.5
    u, v, w = coords(rng, n)
    comps = gridhip.components([l0], [m0], [S])
    vis = ctx.dft_predict((dev(u), dev(v), dev(w)), dev(comps))
    out = host(ctx.phase_shift((dev(u), dev(v), dev(w)), vis, rot(l0, m0), coords=False))
    print(f"worst |shifted - S| / S {np.abs(out - S).max() / S:.3e}")
    assert np.abs(out - S).max() <= 1e-10 * S


def test_shifting_a_prediction_is_predicting_the_rotated_catalogue(ctx):
    import gridhip
    rng = np.random.default_rng(10)
    n, C_, T = 400, 12, 3
    R = rot(0.02, 0.035)
    u, v, w = coords(rng, n, 5e4)
    x = rng.uniform(-0.2, 0.2, n)
    l, m = rng.uniform(-0.04, 0.04, (2, C_))
    flux = rng.normal(size=C_) * 10.0 ** rng.integers(-2, 2, C_)  # both signs, four decades
    spectral = rng.normal(size=(C_, 2)) * 0.5
    s = R @ np.stack([l, m, np.sqrt(1.0 - l * l - m * m)])
    before, after = gridhip.components(l, m, flux, spectral), gridhip.components(s[0], s[1], flux, spectral)
    uvw = (dev(u), dev(v), dev(w))
    vis = ctx.dft_predict(uvw, dev(before), x=dev(x), terms=T)
    shifted, uvw1 = ctx.phase_shift(uvw, vis, R)
    direct = ctx.dft_predict(uvw1, dev(after), x=dev(x), terms=T)
    scale = dft_ref.flux_scale(before, T, x, n)
    err = np.abs(host(shifted) - host(direct))
    print(f"worst |shifted - direct| / sum |S| {np.max(err / scale):.3e}")
    assert (err <= 2e-10 * scale).all()


# ---- averaging ---------------------------------------------------------------------------------------------------------------
def run_avg(ctx, form, group, G, u, v, w, vis, x=None, wt=None, R=None):
    """-> (u_g, v_g, w_g, x_g, vis_g, wt_g, count, stats) as numpy arrays, in the order of average_ref.average"""
    cv = dev if form == "dev" else (lambda a: a)
    back = host if form == "dev" else np.asarray
    uvw = (cv(u), cv(v), cv(w)) if form != "strided" else dev(np.stack([u, v, w], axis=1))
    if form == "strided":
        cv, back = dev, host
    uvw_g, vis_g, wt_g, x_g, cnt, st = ctx.average(uvw, cv(vis), cv(group), G if group is not None else None, weights=cv(wt),
                                                   x=cv(x), R=R, counts=True, stats=True)
    uvw_g = back(uvw_g)
    return (uvw_g[:, 0], uvw_g[:, 1], uvw_g[:, 2], np.zeros(G) if x_g is None else back(x_g), back(vis_g), back(wt_g),
            back(cnt), back(st))


NAMES = ("u", "v", "w", "x", "vis", "weight", "count", "stats")


def same(what, got, want):
    for name, a, b in zip(NAMES, got, want):
        assert A.same_bits(a, b), f"{what}: {name} differs at {np.flatnonzero(np.asarray(a).ravel() != np.asarray(b).ravel())[:8]}"


def every_way(ctx, what, group, G, u, v, w, vis, x=None, wt=None, forms=("dev", "strided", "host")):
    """the reference once; then the device form, the device form on an interleaved (n, 3) array, the host form, a second
    run and a permuted stream: equal bits throughout"""
    want = A.average(group, G, u, v, w, vis, x, wt)
    print(f"{what}: stats {want[7]}")
    for form in forms:
        same(f"{what} [{form}]", run_avg(ctx, form, group, G, u, v, w, vis, x, wt), want)
    same(f"{what} [second run]", run_avg(ctx, "dev", group, G, u, v, w, vis, x, wt), want)
    p = np.random.default_rng(len(u)).permutation(len(u))
    pick = lambda a: None if a is None else np.asarray(a)[p]  # noqa: E731
    same(f"{what} [permuted]", run_avg(ctx, "dev", pick(group), G, u[p], v[p], w[p], vis[p], pick(x), pick(wt)), want)
    return want


def stream(rng, n, G, flags=True):
    u, v, w = rng.normal(size=(3, n)) * 1e3
    vis = noise(rng, n) * 10.0 ** rng.integers(-4, 5, n)
    wt = rng.uniform(0.1, 3.0, n)
    if flags:
        wt[rng.random(n) < 0.05] = 0.0
    return rng.integers(0, G, n), u, v, w, vis, rng.uniform(-1, 1, n), wt


@pytest.mark.parametrize("G", [1, 2, 64, 65, 1000])
@pytest.mark.parametrize("n", SIZES)
def test_average_against_the_reference(ctx, n, G):
    rng = np.random.default_rng(1000 * n + G)
    grp, u, v, w, vis, x, wt = stream(rng, n, G)
    every_way(ctx, f"n {n} G {G}", grp, G, u, v, w, vis, x, wt)


def test_no_visibilities_and_no_group_array(ctx):
    z = np.zeros(0)
    want = every_way(ctx, "n = 0", np.zeros(0, dtype=i64), 3, z, z, z, z.astype(c128))
    assert want[7].tolist() == [0] * 8 and not want[5].any() and not np.signbit(want[5]).any()
    rng = np.random.default_rng(11)
    _, u, v, w, vis, x, wt = stream(rng, 100, 1)
    every_way(ctx, "group None", None, 1, u, v, w, vis, None, None)


@pytest.mark.parametrize("order", ["sorted", "interleaved", "shuffled"])
def test_every_group_size_at_which_L_changes(ctx, order):
    """n_g in {0, 1, 2, 3, 4, 5, 1024, 1025}.  sorted: the neighbours of a wave share a group, and the runs of 1024 and 1025
    cross waves and work-groups; interleaved: the groups at a stride, the neighbours never share one."""
    sizes = [0, 1, 2, 3, 4, 5, 1024, 1025]
    grp = np.concatenate([np.full(k, g) for g, k in enumerate(sizes)])
    rng = np.random.default_rng(12)
    if order == "interleaved":
        grp = np.r_[np.tile([6, 7], 1024), 7, grp[grp < 6][::-1]]
    elif order == "shuffled":
        rng.shuffle(grp)
    n = len(grp)
    _, u, v, w, vis, x, wt = stream(rng, n, 1, flags=False)
    want = every_way(ctx, f"group sizes, {order}", grp, len(sizes), u, v, w, vis, x, wt)
    assert want[6].tolist() == sizes and want[7][5] == 1025 and want[7][0] == 7


def test_runs_between_other_groups_and_flags_inside_a_run(ctx):
    """runs of every length from 1 to 130 of alternating groups, with flagged and left-out samples inside the runs: the
    segmented reduction must cut at each"""
    rng = np.random.default_rng(13)
    grp = np.concatenate([np.full(k, k % 5) for k in range(1, 131)])
    n = len(grp)
    _, u, v, w, vis, x, wt = stream(rng, n, 1, flags=False)
    wt[rng.random(n) < 0.1] = 0.0
    grp[rng.random(n) < 0.1] = -3
    every_way(ctx, "runs", grp, 5, u, v, w, vis, x, wt, forms=("dev",))


def test_one_group_of_a_million(ctx):
    rng = np.random.default_rng(14)
    n = 1 << 20
    _, u, v, w, vis, x, wt = stream(rng, n, 1)
    want = A.average(None, 1, u, v, w, vis, x, wt)
    got = run_avg(ctx, "dev", None, 1, u, v, w, vis, x, wt)
    same("n = 2^20, G = 1", got, want)
    assert want[7][5] == want[6][0] > 900000


def test_special_values(ctx):
    """ids out of range and negative, a fully flagged group, weights of 0, negative and NaN, an Inf visibility, a product
    that overflows, 1e-300 beside 1e300 in one group, denormals, -0.0"""
    grp = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 9, -1, 1 << 40, 5, 5, 6, 6, 6], dtype=i64)
    n, G = len(grp), 8                                                 # (group 7 is empty)
    vis = np.ones(n, dtype=c128)
    wt, u = np.ones(n), np.arange(1.0, n + 1)
    v, w, x = -u, 0.5 * u, u * u
    wt[[0, 1, 2]] = [0.0, -1.0, np.nan]                                # group 0: fully flagged
    vis[3], vis[4] = np.inf, 1e300 + 0j                                # group 1: an Inf, and 1e300 * 1e10 overflows
    wt[4] = 1e10
    vis[6], vis[7] = 1e-300 + 1e300j, 1e300 + 1e-300j                  # group 2: 1e-300 beside 1e300
    vis[[8, 9, 10]] = [5e-324 + 1e-310j, -1e-310 + 5e-324j, 2e-320]    # group 3: denormals
    wt[[8, 9, 10]] = [1.0, 0.5, 0.25]
    vis[[11, 12, 13, 14]] = [-0.0, complex(0.0, -0.0), complex(-0.0, -0.0), 0.0]  # group 4: zeros of both signs
    u[[11, 12, 13, 14]] = -0.0
    u[18], x[19] = np.nan, np.inf                                      # group 5: a NaN coordinate, an Inf x: not finite
    wt[[20, 21, 22]] = [1e-300, 1e300, 5e-324]                         # group 6: the weights themselves span the range
    want = every_way(ctx, "special values", grp, G, u, v, w, vis, x, wt)
    cnt, st = want[6], want[7]
    assert cnt.tolist() == [0, 1, 2, 3, 4, 0, 3, 0]
    assert st.tolist() == [5, 13, 3, 3, 4, 4, 0, 0]
    assert want[5][[0, 5, 7]].tolist() == [0.0, 0.0, 0.0] and not np.signbit(want[5]).any()
    assert want[4][2] == complex(0.5e300, 0.5e300) and want[4][4] == 0 and not np.signbit(want[0][4])


def test_the_fused_shift_is_the_two_calls(ctx):
    """average(R=...) against phase_shift followed by average, both on the device: the same bits, stats[6] included"""
    rng = np.random.default_rng(15)
    R = rot(0.03, 0.01)
    for n, G, form in ((257, 5, "dev"), (3000, 40, "strided"), (64, 1, "dev")):
        grp, u, v, w, vis, x, wt = stream(rng, n, G)
        u[n // 2], grp[0] = np.nan, -1
        u, v, w = u * 50, v * 50, w * 50
        out, uvw1, st = ctx.phase_shift((dev(u), dev(v), dev(w)), dev(vis), R, stats=True)
        u1, v1, w1 = (host(uvw1)[:, i].copy() for i in range(3))
        two = list(run_avg(ctx, form, grp, G, u1, v1, w1, host(out), x, wt))
        two[7] = two[7].copy()
        two[7][6] = host(st)[1]
        one = run_avg(ctx, form, grp, G, u, v, w, vis, x, wt, R=R)
        same(f"fused n {n} G {G}", one, two)
        assert one[7][6] == 1 and one[7][4] >= 1
        if form == "dev":
            same(f"fused n {n} G {G} [host]", run_avg(ctx, "host", grp, G, u, v, w, vis, x, wt, R=R), two)


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def observation(rng, A_, times):
    p, q = np.triu_indices(A_, 1)
    pos = rng.uniform(-100, 100, (A_, 2))
    us, vs = [], []
    for t in range(times):
        ang = 0.01 * t
        b = (pos[p] - pos[q]) @ np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]).T
        us.append(b[:, 0]), vs.append(b[:, 1])
    a1, a2 = np.tile(p, times), np.tile(q, times)
    return np.concatenate(us), np.concatenate(vs), a1, a2, np.repeat(np.arange(times), len(p))


def test_average_feeds_gaincal_and_an_imager(ctx):
    """8 antennas, 16 times averaged by 4 per baseline: a unit point at the centre seen through gains g is g_p conj(g_q) at
    every time, so the averaged stream solves to the same gains, and an imager takes its (G, 3) baselines, weights and
    visibilities as they come"""
    import torch
    import gridhip
    rng = np.random.default_rng(16)
    A_, times = 8, 16
    u, v, a1, a2, t = observation(rng, A_, times)
    n = len(u)
    g = (1 + 0.2 * rng.normal(size=A_)) * np.exp(1j * rng.uniform(-1, 1, A_))
    vis = g[a1] * np.conj(g[a2])
    grp, G, g1, g2 = gridhip.average_groups(dev(a1), dev(a2), dev(t), ntime=4)
    assert G == 28 * 4
    uvw_g, vis_g, wt_g, _, cnt = ctx.average((dev(u), dev(v), dev(np.zeros(n))), dev(vis), grp, G, counts=True)
    assert host(cnt).tolist() == [4] * G and host(wt_g).tolist() == [4.0] * G
    gains, stats = ctx.gaincal(vis_g, torch.ones_like(vis_g), g1, g2, A_, weights=wt_g, niter=200, tol=1e-9)
    got = host(gains)[0]
    assert np.abs(got - g * np.exp(-1j * np.angle(g[0]))).max() < 1e-6
    theta, lam = 0.1, 640
    im = ctx.imager(theta, lam, uvw_g, ("simple",), weighting="natural", weights=wt_g)
    cal, _ = ctx.apply_gains(gains, vis_g, g1, g2)
    img = host(im.cycle(cal))
    N = ctx.image_size(theta, lam)
    assert np.isfinite(img).all() and np.unravel_index(np.argmax(img), img.shape) == (N // 2, N // 2)
    im.close()


def test_a_captured_shift_and_average_replays_to_the_same_bits(ctx):
    import torch
    rng = np.random.default_rng(17)
    n, G, R = 5000, 37, rot()
    grp, u, v, w, vis, x, wt = stream(rng, n, G)
    m, dvis, dg, dx, dw = dev(np.stack([u, v, w], axis=1) * 20), dev(vis), dev(grp), dev(x), dev(wt)

    def step():
        out, uvw1 = ctx.phase_shift(m, dvis, R)
        return ctx.average(uvw1, out, dg, G, weights=dw, x=dx, counts=True, stats=True)

    eager = []
    for scale in (1.0, 0.5):
        dvis.copy_(dev(vis * scale))
        eager.append([host(a) for a in step()])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        res = step()
    torch.cuda.synchronize()
    for i, scale in enumerate((1.0, 0.5)):
        dvis.copy_(dev(vis * scale))
        for a in res:
            a.fill_(7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("uvw", "vis", "weight", "x", "count", "stats"), res, eager[i]):
            assert A.same_bits(host(a), b), name
    fused = [host(a) for a in ctx.average(m, dvis, dg, G, weights=dw, x=dx, R=R, counts=True, stats=True)]
    for a, b in zip(fused[:5], eager[1][:5]):
        assert A.same_bits(a, b)
