"""Direct-Fourier prediction on the GPU (gridhip_dft_predict[_dev], gridhip_components_from_image[_dev]; Context.dft_predict,
Context.components_from_image) against the numpy restatement tests/dft_ref.py.  The bound everywhere is dft_ref.TOL = 1e-10
times the sum of the component fluxes |S_c(x)|: three roundings of a phase of at most 1e4 turns cost 2e-11 of it, and the
reference evaluates the phase in long double.  Inputs keep |u l| + |v m| + |w (n - 1)| <= 1e4."""
import ctypes as C

import numpy as np
import pytest

import dft_ref
import gaincal_ref

pytestmark = pytest.mark.gpu

WG_VIS = 512  # the visibilities of a work-group of the main kernel (two per thread)
CHUNK = 256   # the components it stages in LDS at a time


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.cpu().numpy()


def stream(n, seed):
    """u, v, w, x: |u l| + |v m| <= 8e3 and |w (n - 1)| <= 1e3 for the components of `catalogue`"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2e4, 2e4, n), rng.uniform(-2e4, 2e4, n), rng.uniform(-2e4, 2e4, n), rng.uniform(-0.3, 0.3, n)


def catalogue(C_, seed, gauss=True):
    """points mixed with Gaussians: every third a Gaussian with a bpa that is no multiple of pi / 2, every sixth with bmin = 0"""
    rng = np.random.default_rng(seed)
    c = np.zeros((C_, 10))
    c[:, 0], c[:, 1] = rng.uniform(-0.2, 0.2, C_), rng.uniform(-0.2, 0.2, C_)
    c[:, 2:6] = rng.normal(size=(C_, 4))
    if gauss:
        g = np.arange(C_) % 3 == 1
        c[g, 6] = rng.uniform(1e-5, 5e-5, g.sum())
        c[g, 7] = c[g, 6] * rng.uniform(0.2, 1.0, g.sum())
        c[g & (np.arange(C_) % 6 == 1), 7] = 0.0
        c[g, 8] = rng.uniform(0.1, 1.4, g.sum()) + (np.pi / 2) * rng.integers(0, 4, g.sum())
    return c


def check(got, comps, u, v, w=None, x=None, T=1, count=None, vis_sub=None, stats=None):
    ref, st = dft_ref.dft_predict(comps, u, v, w, x, T, count, vis_sub)
    used = comps if count is None else comps[:min(max(int(count), 0), len(comps))]
    scale = dft_ref.flux_scale(used, T, x, len(u))
    err = np.abs(got - ref)
    worst = (err / np.maximum(scale, 1e-300)).max() if len(u) else 0.0
    print(f"n {len(u)} C {len(comps)} T {T}: worst error {worst:.2e} of the flux")
    assert (err <= dft_ref.TOL * scale).all()
    if stats is not None:
        assert list(stats[:3]) == list(st)
    return ref


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, WG_VIS - 1, WG_VIS, WG_VIS + 1])
def test_parity_over_visibility_counts(ctx, n):
    comps = catalogue(5, 1)
    u, v, w, x = stream(n, n)
    got, st = ctx.dft_predict((u, v, w), comps, x=x, terms=2, stats=True)
    check(got, comps, u, v, w, x, 2, stats=st)
    assert st[3] == 1


@pytest.mark.parametrize("C_,n", [(0, 65), (1, 65), (CHUNK - 1, 65), (CHUNK, 65), (CHUNK + 1, 65), (2 * CHUNK + 3, 130)])
def test_parity_over_component_counts(ctx, C_, n):
    comps = catalogue(C_, 2)
    u, v, w, _ = stream(n, 3)
    got, st = ctx.dft_predict((u, v, w), comps, stats=True)
    ref = check(got, comps, u, v, w, stats=st)
    if C_ == 0:
        assert np.array_equal(got, np.zeros(n)) and np.array_equal(ref, got)
        sub = np.full(n, 1 - 2j)
        assert np.array_equal(ctx.dft_predict((u, v, w), comps, vis_sub=sub), sub)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("with_x", [False, True])
def test_parity_over_terms(ctx, T, with_x):
    comps = catalogue(40, 4)
    u, v, w, x = stream(130, 5)
    x = x if with_x else None
    got = ctx.dft_predict((u, v, w), comps, x=x, terms=T)
    check(got, comps, u, v, w, x, T)


def test_parity_over_forms(ctx):
    """uv_stride 1 and 3, w NULL, the residual form and the residual form in place, host and device"""
    import torch
    comps = catalogue(30, 6)
    n = 300
    u, v, w, x = stream(n, 7)
    pred = ctx.dft_predict((u, v, w), comps, x=x, terms=3)
    check(pred, comps, u, v, w, x, 3)
    uvw = np.stack([u, v, w], axis=1)
    assert np.array_equal(ctx.dft_predict(uvw, comps, x=x, terms=3), pred)  # (the same sums from a stride of 3)
    check(ctx.dft_predict((u, v, None), comps, x=x, terms=3), comps, u, v, None, x, 3)
    rng = np.random.default_rng(8)
    sub = rng.normal(size=n) + 1j * rng.normal(size=n)
    res = ctx.dft_predict((u, v, w), comps, x=x, terms=3, vis_sub=sub)
    check(res, comps, u, v, w, x, 3, vis_sub=sub)
    buf = sub.copy()
    assert ctx.dft_predict((u, v, w), comps, x=x, terms=3, vis_sub=buf, out=buf) is buf and np.array_equal(buf, res)
    # the device forms: the same kernels, so the same bits
    dc, dx, dsub = dev(comps), dev(x), dev(sub)
    d = ctx.dft_predict(dev(uvw), dc, x=dx, terms=3)
    assert d.is_cuda and np.array_equal(host(d), pred)
    dbuf, duvw = dsub.clone(), (dev(u), dev(v), dev(w))
    ctx.dft_predict(duvw, dc, x=dx, terms=3, vis_sub=dbuf, out=dbuf)
    assert np.array_equal(host(dbuf), res)
    # a second device call takes no memory
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    ctx.dft_predict(duvw, dc, x=dx, terms=3, vis_sub=dbuf, out=dbuf)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free


@pytest.mark.parametrize("C_", [7, 2])
def test_slices(ctx, C_):
    """"dft_slices" = 3: C = 7 gives slices of 3, 3 and 1 components, C = 2 an empty third slice"""
    comps = catalogue(C_, 9)
    u, v, w, x = stream(WG_VIS + 37, 10)
    rng = np.random.default_rng(11)
    sub = rng.normal(size=len(u)) + 1j * rng.normal(size=len(u))
    one, st1 = ctx.dft_predict((u, v, w), comps, x=x, terms=2, stats=True)
    ctx.set_option("dft_slices", 3)
    try:
        a, st = ctx.dft_predict((u, v, w), comps, x=x, terms=2, stats=True)
        b = ctx.dft_predict((u, v, w), comps, x=x, terms=2)
        r = ctx.dft_predict((u, v, w), comps, x=x, terms=2, vis_sub=sub)
    finally:
        ctx.set_option("dft_slices", 0)
    assert st1[3] == 1 and st[3] == 3 and list(st[:3]) == list(st1[:3])
    assert a.tobytes() == b.tobytes()
    check(a, comps, u, v, w, x, 2)
    assert (np.abs(a - one) <= dft_ref.TOL * dft_ref.flux_scale(comps, 2, x, len(u))).all()
    check(r, comps, u, v, w, x, 2, vis_sub=sub)


@pytest.mark.parametrize("count", [0, 3, 9, 12, -4])
def test_count_on_the_device(ctx, count):
    """min(max(count, 0), C) components are used, and the rows after them - NaN here - are never read"""
    import torch
    C_ = 9
    comps = catalogue(C_, 12)
    u, v, w, _ = stream(70, 13)
    k = min(max(count, 0), C_)
    poisoned = comps.copy()
    poisoned[k:] = np.nan
    dcount = torch.tensor([count], dtype=torch.int64, device="cuda")
    got, st = ctx.dft_predict((dev(u), dev(v), dev(w)), dev(poisoned), count=dcount, stats=True)
    got, st = host(got), host(st)
    check(got, comps, u, v, w, count=count, stats=st)
    assert st[0] == k and st[1] == 0
    clean = ctx.dft_predict((u, v, w), comps[:k])
    assert np.array_equal(got, clean)  # the same sum in the same order
    assert np.array_equal(ctx.dft_predict((u, v, w), poisoned, count=count), clean)  # the host form takes a number


def test_skipped_components(ctx):
    """each kind of skipped component next to valid ones contributes exactly 0 and is counted"""
    base = catalogue(6, 14)
    u, v, w, x = stream(90, 15)
    want = ctx.dft_predict((u, v, w), base, x=x, terms=2)
    kinds = []
    for field in (0, 1, 2, 3, 6, 7, 8):  # a NaN or Inf in any read field (T = 2: f0, f1)
        row = catalogue(1, 16)[0]
        row[6:9] = 3e-5, 1e-5, 0.4
        row[field] = np.nan if field % 2 == 0 else np.inf
        kinds.append(row)
    far, swapped, negative = catalogue(1, 17)[0], catalogue(1, 18)[0], catalogue(1, 19)[0]
    far[0], far[1] = 0.8, 0.7                 # r2 > 1
    swapped[6:9] = 1e-5, 2e-5, 0.3            # bmaj < bmin
    negative[6:9] = 1e-5, -1e-5, 0.3          # a negative axis
    huge = catalogue(1, 23)[0]
    huge[6:9] = 1e160, 1e-5, 0.3              # a finite axis whose square overflows: the Gaussian's form is not finite
    kinds += [far, swapped, negative, huge]
    for i, row in enumerate(kinds):
        comps = np.insert(base, 3, row, axis=0)
        got, st = ctx.dft_predict((u, v, w), comps, x=x, terms=2, stats=True)
        assert np.array_equal(got, want), i
        assert list(st[:3]) == [6, 1, 0], i
        assert list(dft_ref.skipped(comps, 2)) == [False] * 3 + [True] + [False] * 3
    # f2 and f3 are not read with T = 2: a NaN there changes nothing
    comps = base.copy()
    comps[:, 4:6] = np.nan
    got, st = ctx.dft_predict((u, v, w), comps, x=x, terms=2, stats=True)
    assert np.array_equal(got, want) and st[1] == 0
    check(want, base, u, v, w, x, 2)


def test_non_finite_visibilities(ctx):
    """a NaN or Inf u, v, w or x predicts exactly 0 (vis_sub[k] in the residual form) and is counted; its neighbours in
    the same thread (k +- 256) and the same wave are right"""
    comps = catalogue(8, 20)
    n = 2 * WG_VIS
    u, v, w, x = stream(n, 21)
    badk = [3, 70, 256 + 5, 513, 900]
    u[3], v[70], w[256 + 5], x[513], u[900] = np.nan, np.inf, -np.inf, np.nan, np.inf
    rng = np.random.default_rng(22)
    sub = rng.normal(size=n) + 1j * rng.normal(size=n)
    got, st = ctx.dft_predict((u, v, w), comps, x=x, terms=3, stats=True)
    check(got, comps, u, v, w, x, 3, stats=st)
    assert st[2] == 5 and np.array_equal(got[badk], np.zeros(5))
    res = ctx.dft_predict((u, v, w), comps, x=x, terms=3, vis_sub=sub)
    assert np.array_equal(res[badk], sub[badk])
    check(res, comps, u, v, w, x, 3, vis_sub=sub)
    # without x its NaN is not looked at; with C = 0 the count is still made
    _, st = ctx.dft_predict((u, v, w), comps, terms=3, stats=True)
    assert st[2] == 4
    z, st = ctx.dft_predict((u, v, w), comps[:0], x=x, stats=True)
    assert st[2] == 5 and not z.any()


@pytest.mark.parametrize("N", [16, 15])
def test_convention_against_predict(ctx, N):
    """components_from_image then dft_predict at the integer cells is Context.predict's simple kind"""
    theta, lam = 0.05, 20 * N
    assert ctx.image_size(theta, lam) == N
    rng = np.random.default_rng(N)
    model = np.zeros((N, N))
    cells = rng.choice(N * N, 5, replace=False)
    model.ravel()[cells] = rng.normal(size=5)
    iy, ix = np.mgrid[0:N, 0:N]
    u, v = ((ix - N // 2) / theta).ravel(), ((iy - N // 2) / theta).ravel()
    comps, count = ctx.components_from_image(theta, lam, model, 8)
    assert count == 5
    got = ctx.dft_predict((u, v, None), comps, count=count)
    want = ctx.predict(theta, lam, (u, v, np.zeros_like(u)), model, ("simple",))
    assert np.abs(want).max() > 0.1
    assert np.abs(got - want).max() <= 1e-10 * np.abs(model).sum()


def test_sign_of_w(ctx):
    """one off-centre pixel at test_gpu_predict's shape: the library's DFT is at least 10 x closer to the w_cache
    prediction (its w-kernels' truncation is the distance) than the reference evaluated with w negated.  At integer
    cells, so that the distance is the w term's alone and not the rounding of u, v to the oversampled grid.  On the
    numpy references the two distances are 0.0041 and 0.105 rms."""
    from test_gpu_predict import KO, SHAPES
    theta, lam = SHAPES[0]
    N = 64
    rng = np.random.default_rng(5)
    n = 200
    u, v = rng.integers(-24, 25, n) / theta, rng.integers(-24, 25, n) / theta
    w = rng.uniform(-300.0, 300.0, n)
    model = np.zeros((N, N))
    model[36, 27] = 1.0
    wc = ctx.predict(theta, lam, (u, v, w), model, ("w_cache", KO))
    comps, count = ctx.components_from_image(theta, lam, model, 1)
    got = ctx.dft_predict((u, v, w), comps)
    wrong = dft_ref.dft_predict(comps, u, v, w, wsign=-1.0)[0]
    right, other = np.sqrt((np.abs(got - wc) ** 2).mean()), np.sqrt((np.abs(wrong - wc) ** 2).mean())
    print(f"rms distance to w_cache: dft {right:.4f}, w negated {other:.4f}")
    assert count == 1 and 10 * right <= other


@pytest.mark.parametrize("N", [4, 5, 33])
@pytest.mark.parametrize("T", [1, 3])
def test_components_from_image(ctx, N, T):
    theta, lam = 0.01 * N, 100
    assert ctx.image_size(theta, lam) == N
    rng = np.random.default_rng(100 * N + T)
    model = np.where(rng.uniform(size=(T, N, N)) < 0.3, rng.normal(size=(T, N, N)), 0.0)
    model[:, 0, 0] = 0.0
    model[T - 1, 0, 0] = 2.5  # (for T = 3: non-zero in the last term only)
    model[:, N - 1, N - 1] = 0.0
    model[0, N - 1, N - 1] = -1.0
    want = dft_ref.components_from_image(theta, model)
    found = len(want)
    m = model if T > 1 else model[0]
    comps, count = ctx.components_from_image(theta, lam, m, found + 3)
    assert count == found and comps.shape == (found + 3, 10)
    # l, m: a product and a quotient, each correctly rounded - the same two operations as the reference's
    assert np.array_equal(comps[:found], want) and not comps[found:].any()
    assert np.array_equal(comps[0, :2], dft_ref.pixel_lm(theta, N, 0, 0)) and comps[0, 2 + T - 1] == 2.5
    # max_c below the number found: exactly max_c rows, the full count, the rest untouched
    few = found // 2
    out = np.full((few + 2, 10), -7.0)
    c2, count2 = ctx.components_from_image(theta, lam, m, few, out=out[:few])
    assert count2 == found and np.array_equal(out[:few], want[:few]) and (out[few:] == -7.0).all()
    # the same on the device, where the rows after max_c are the caller's own memory: the tail keeps its bytes
    import torch
    dout = torch.full((few + 2, 10), -7.0, dtype=torch.float64, device="cuda")
    tail = host(dout[few:]).tobytes()
    _, dcount = ctx.components_from_image(theta, lam, dev(m), few, out=dout[:few])
    assert int(dcount[0]) == found and np.array_equal(host(dout[:few]), want[:few]) and host(dout[few:]).tobytes() == tail
    # the device form: the same bytes, twice, and a count that stays on the device
    d1, n1 = ctx.components_from_image(theta, lam, dev(m), found + 3)
    d2, n2 = ctx.components_from_image(theta, lam, dev(m), found + 3)
    assert n1.is_cuda and int(n1[0]) == found and int(n2[0]) == found
    assert host(d1).tobytes() == host(d2).tobytes() == comps.tobytes()
    dz, nz = ctx.components_from_image(theta, lam, dev(np.zeros_like(m)), 4)
    assert int(nz[0]) == 0 and not host(dz).any()
    assert ctx.components_from_image(theta, lam, np.zeros_like(m), 0)[1] == 0


def test_components_across_segments(ctx):
    """more cells than one segment of the compaction (1024), more than one work-group: order and count hold"""
    theta, lam, N = 0.7, 100, 70
    rng = np.random.default_rng(70)
    model = np.where(rng.uniform(size=(2, N, N)) < 0.4, rng.normal(size=(2, N, N)), 0.0)
    want = dft_ref.components_from_image(theta, model)
    comps, count = ctx.components_from_image(theta, lam, model, len(want))
    assert count == len(want) > 1024 and np.array_equal(comps, want)


def test_refusals(ctx):
    """every GRIDHIP_EINVAL case of the header, through the C ABI on device arrays: vis_out, comps and count stay the bytes
    they were"""
    import torch
    from gridhip import _lib
    lib = _lib.load()
    n, C_, N = 40, 6, 8
    theta, lam = 0.08, 100
    u, v, w, x = (dev(a) for a in stream(n, 30))
    comps, sub = dev(catalogue(C_, 31)), dev(np.ones(n, dtype=np.complex128))
    cnt = torch.tensor([C_], dtype=torch.int64, device="cuda")
    out = torch.full((n,), 7 - 7j, dtype=torch.complex128, device="cuda")
    model = dev(np.ones((2, N, N)))
    clist = torch.full((5, 10), -3.0, dtype=torch.float64, device="cuda")
    ccount = torch.tensor([-9], dtype=torch.int64, device="cuda")
    stats = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
    keep = [host(t).tobytes() for t in (out, clist, ccount, stats)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    h = ctx._h
    ctx._use_torch_stream()

    def predict(c=h, C__=C_, comps_=comps, count=cnt, T=2, n_=n, u_=u, v_=v, w_=w, stride=1, x_=x, sub_=sub, out_=out,
                stats_=stats):
        return lib.gridhip_dft_predict_dev(c, C__, p(comps_), p(count), T, n_, p(u_), p(v_), p(w_), stride, p(x_), p(sub_),
                                           p(out_), p(stats_))

    def from_image(c=h, T=2, model_=model, max_c=5, comps_=clist, count=ccount):
        return lib.gridhip_components_from_image_dev(c, theta, lam, T, p(model_), max_c, p(comps_), p(count))

    inside = out.view(torch.float64)[2:]  # (a view into vis_out: an overlap that is not vis_sub itself)
    refused = [predict(c=None), predict(n_=-1), predict(C__=-1), predict(T=0), predict(T=5), predict(comps_=None),
               predict(u_=None), predict(v_=None), predict(out_=None), predict(stride=0),
               predict(u_=inside), predict(v_=inside), predict(w_=inside), predict(x_=inside), predict(comps_=inside),
               predict(count=out.view(torch.int64)[4:]), predict(sub_=out.view(torch.float64)[2:].view(torch.complex128)),
               predict(stats_=inside), predict(stats_=comps.view(-1)[3:]), predict(stats_=cnt.view(torch.float64)),
               predict(stats_=u[5:]), predict(stats_=x[n - 1:]), predict(stats_=sub.view(torch.float64)[8:]),
               from_image(c=None), from_image(T=0), from_image(T=5), from_image(model_=None), from_image(max_c=-1),
               from_image(count=None), from_image(comps_=None), from_image(comps_=model), from_image(count=model)]
    assert refused == [_lib.EINVAL] * len(refused)
    assert lib.gridhip_components_from_image_dev(h, 0.0, lam, 1, p(model), 5, p(clist), p(ccount)) == _lib.EINVAL
    torch.cuda.synchronize()
    assert [host(t).tobytes() for t in (out, clist, ccount, stats)] == keep
    # the host forms refuse alike and leave host arrays alone
    hout, hcomps, hcount = np.full(n, 7 - 7j), np.full((5, 10), -3.0), np.array([-9], dtype=np.int64)
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    hu = host(u)
    assert lib.gridhip_dft_predict(h, C_, hp(host(comps)), None, 9, n, hp(hu), hp(hu), None, 1, None, None, hp(hout), None) \
        == _lib.EINVAL
    assert lib.gridhip_components_from_image(h, theta, lam, 2, hp(host(model)), -1, hp(hcomps), hp(hcount)) == _lib.EINVAL
    assert (hout == 7 - 7j).all() and (hcomps == -3.0).all() and hcount[0] == -9
    # and the valid edges: n = 0 and C = 0
    assert predict(n_=0, u_=None, v_=None, out_=None, x_=None, sub_=None, w_=None) == 0
    assert predict(C__=0, comps_=None, count=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host(out), host(sub)) and list(host(stats)) == [0, 0, 0, 1]


def test_a_captured_prediction_and_solve_replay_to_the_eager_results(ctx):
    """dft_predict with a device count, then gaincal against it, as one graph; replayed with other components"""
    import torch
    theta, lam, N, A, u, v, a1, a2, comps, model, gt = dft_ref.selfcal_observation()
    n = len(u)
    exact = dft_ref.dft_predict(comps, u, v)[0]
    vis = dev(gaincal_ref.apply_gains(gt, exact, a1, a2, inverse=False)[0])
    du, dv, d1, d2 = dev(u), dev(v), dev(a1), dev(a2)
    lists = [comps * np.r_[1, 1, s, np.ones(7)][None, :] for s in (1.0, 0.5, 2.0)]
    padded = [np.concatenate([c, np.full((2, 10), np.nan)]) for c in lists]
    dcomps, dcount = dev(padded[0]), torch.tensor([3], dtype=torch.int64, device="cuda")
    kw = dict(niter=30, tol=0.0)

    def step(out, gains):
        ctx.dft_predict((du, dv, None), dcomps, count=dcount, out=out)
        return ctx.gaincal(vis, out, d1, d2, A, gains=gains, **kw)

    eager = []
    for c in padded:
        dcomps.copy_(dev(c))
        mv = torch.empty(n, dtype=torch.complex128, device="cuda")
        g, s = step(mv, None)
        eager.append((host(mv), host(g), host(s)))
    mv = torch.empty(n, dtype=torch.complex128, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # warm-up on the capture stream: the pool then holds every block
        step(mv, None)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):  # one linear chain: no parallel branches
        ctx.dft_predict((du, dv, None), dcomps, count=dcount, out=mv)
        g, stats = ctx.gaincal(vis, mv, d1, d2, A, **kw)
    torch.cuda.synchronize()
    for i in (1, 2):
        dcomps.copy_(dev(padded[i]))
        mv.fill_(7.0), g.fill_(7.0), stats.fill_(7.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        M, G, S = eager[i]
        assert np.array_equal(host(mv), M)  # the prediction is the same bits on every run
        assert np.abs(host(g) - G).max() <= 1e-9 * np.abs(G).max()
        assert S[0] == 30 and np.array_equal(host(stats)[[0, 4, 5, 6, 7]], S[[0, 4, 5, 6, 7]])


def test_selfcal_against_the_exact_model(ctx):
    """Three point sources off pixel centres, 8 antennas, all 28 baselines at 4 times; the data are the DFT of the sources
    corrupted by known gains.  The solve against dft_predict matches gaincal_ref on dft_ref's model to the gaincal suite's
    1e-9, and ends at a chi^2 far below the one the same solve reaches against Context.predict(("simple",)) of the
    pixelised sources: on the numpy references (tests/test_dft_host.py) 4.168e-11 against 341.1, ratio 1.222e-13, asserted
    here with a 10 x margin."""
    theta, lam, N, A, u, v, a1, a2, comps, model, gt = dft_ref.selfcal_observation()
    exact_ref = dft_ref.dft_predict(comps, u, v)[0]
    exact = ctx.dft_predict((u, v, None), comps)
    assert (np.abs(exact - exact_ref) <= dft_ref.TOL * np.abs(comps[:, 2]).sum()).all()
    vis = ctx.apply_gains(gt, exact_ref, a1, a2, inverse=False)[0]
    gA, sA = ctx.gaincal(vis, exact, a1, a2, A, **dft_ref.SELFCAL_SOLVE)
    gR, sR = gaincal_ref.gaincal(vis, exact_ref, a1, a2, A, **dft_ref.SELFCAL_SOLVE)
    assert sA[0] == sR[0] and np.abs(gA - gR).max() <= 1e-9 * np.abs(gR).max()
    simple = ctx.predict(theta, lam, (u, v, np.zeros_like(u)), model, ("simple",))
    gB, sB = ctx.gaincal(vis, simple, a1, a2, A, **dft_ref.SELFCAL_SOLVE)
    print(f"chi2 against the DFT {sA[2]:.4e}, against the pixelised model {sB[2]:.4e}, ratio {sA[2] / sB[2]:.4e}")
    assert sA[2] / sB[2] <= dft_ref.SELFCAL_RATIO
    assert np.abs(gA - gt * np.exp(-1j * np.angle(gt[:, :1]))).max() < 1e-6
