"""CPU checks of the Python binding's host marshalling: what each numpy-path method hands to the C ABI.

A Context is made without a device (as tests/test_aw_imaging_host.py makes it) and its library replaced by a recorder
whose every gridhip_* entry point checks its arguments against an expectation WHILE THE CALL IS IN PROGRESS (the
binding's converted copies only live that long) and returns 0.  The expectations are written from include/gridhip.h:
the function's name, each scalar, and for each pointer the dtype, length and values of the array it addresses - or the
very address of the caller's array where no copy may be made.  Inputs are deliberately awkward: float32 and
non-contiguous arrays, lists, (n, 3) and tuple baselines, None where the ABI allows NULL.
"""
import ctypes as C

import numpy as np
import pytest

THETA, LAM, NPIX = 0.008, 2000, 16  # gridhip_image_size(0.008, 2000) = round(16.0)
N = 6                               # visibilities per call
c128, f64, i64 = np.complex128, np.float64, np.int64


def address(p):
    """the address ctypes passes for this c_void_p argument"""
    if p is None or isinstance(p, int):
        return p
    assert isinstance(p, C.c_void_p), f"{p!r} is not a pointer argument"
    return p.value


def memory(addr, dtype, n):
    return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype)


class Arr:
    """the argument addresses an array of this dtype, length and contents (any shape: compared flat)"""

    def __init__(self, values, dtype):
        self.want = np.array(values, dtype=dtype).ravel()

    def check(self, arg, where):
        got = memory(address(arg), self.want.dtype, self.want.size)
        assert np.array_equal(got, self.want), f"{where}: {got} != {self.want}"


class Same:
    """the argument is the address of the caller's own array (+ offset bytes): passed as it is, not copied"""

    def __init__(self, arr, offset=0):
        self.arr, self.offset = arr, offset

    def check(self, arg, where):
        assert address(arg) == self.arr.ctypes.data + self.offset, f"{where}: not the caller's array"


class Copy(Arr):
    """the contents of the caller's array at another address (the binding protects the caller's array)"""

    def __init__(self, arr, dtype):
        super().__init__(arr, dtype)
        self.arr = arr

    def check(self, arg, where):
        super().check(arg, where)
        assert address(arg) != self.arr.ctypes.data, f"{where}: the caller's own array"


class Out:
    """an output of n elements: the recorder fills it with 1, 2, 3 ..., which the caller must find in what the method
    returns (so the pointer addresses the returned array, and that array is of this dtype and at least this long)"""

    def __init__(self, dtype, n):
        self.fill = np.arange(1, n + 1).astype(dtype)

    def check(self, arg, where):
        memory(address(arg), self.fill.dtype, self.fill.size)[:] = self.fill

    def returned(self, arr, shape):
        assert isinstance(arr, np.ndarray) and arr.dtype == self.fill.dtype and arr.shape == tuple(shape)
        assert arr.flags.c_contiguous and np.array_equal(arr.ravel(), self.fill)
        return True


class Ref:
    """a by-reference scalar output of this ctypes type; the recorder stores `value` in it"""

    def __init__(self, ctype, value):
        self.ctype, self.value = ctype, value

    def check(self, arg, where):
        obj = arg._obj if hasattr(arg, "_obj") else arg.contents
        assert isinstance(obj, self.ctype), f"{where}: {type(obj)}"
        obj.value = self.value


class Recorder:
    """Stands in for the loaded library.  gridhip_image_size is the real one; every other gridhip_* attribute checks the
    call against the expectation set by expect() and returns 0."""

    def __init__(self):
        from gridhip import _lib
        self.gridhip_image_size = _lib.load().gridhip_image_size
        self.calls = []
        self.want = None

    def expect(self, name, handle, spec):
        self.want = (name, handle, spec)

    def __getattr__(self, name):
        if not name.startswith("gridhip_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            if name.endswith("destroy"):
                return 0
            assert self.want is not None, f"unexpected call of {name}"
            want_name, handle, spec = self.want
            self.want = None
            assert name == want_name
            assert args[0] is handle, "first argument: the handle"
            assert len(args) == 1 + len(spec), f"{name}: {len(args) - 1} arguments after the handle, not {len(spec)}"
            for i, (a, s) in enumerate(zip(args[1:], spec)):
                where = f"{name} argument {i + 1}"
                if s is None:
                    assert a is None, where
                elif isinstance(s, int):
                    assert type(a) is int and a == s, f"{where}: {a!r} != {s}"
                elif isinstance(s, float):
                    assert type(a) in (int, float) and a == s, f"{where}: {a!r} != {s}"
                else:
                    s.check(a, where)
            return 0
        return entry


HANDLE = C.c_void_p(0xC0FFEE)


@pytest.fixture
def rig():
    import gridhip
    rec = Recorder()
    ctx = object.__new__(gridhip.Context)
    ctx._lib, ctx._h, ctx.device = rec, HANDLE, 0

    def run(fn, name, *spec, handle=HANDLE):
        before = len(rec.calls)
        rec.expect(name, handle, spec)
        out = fn()
        assert rec.calls[before:] == [name], f"{name}: the calls were {rec.calls[before:]}"
        return out
    yield ctx, rec, run
    ctx._h = None


# ---- inputs, each in an awkward and in the right form ------------------------------------------------------------
def awkward():
    """float32 u, a non-contiguous v, w as a list; an (n, 3) float32 Fortran-ordered matrix of the same baselines"""
    u = (np.arange(N, dtype=np.float32) - 2) / 16
    v = (np.arange(2 * N, dtype=f64) / 32)[::2]
    w = [float(k) * 8 for k in range(N)]
    m = np.asfortranarray(np.stack([u, v, w], axis=1).astype(np.float32))
    assert not v.flags.c_contiguous and not m.flags.c_contiguous
    return u, v, w, m


def cplx(*shape, dtype=np.complex64):
    k = np.arange(int(np.prod(shape)), dtype=f64).reshape(shape)
    return (k - 1j * (k % 5)).astype(dtype)


def strided_vis():
    vis = cplx(2 * N, dtype=c128)[::2]
    assert not vis.flags.c_contiguous
    return vis


WBIN = [1, 0, 1, 1, 0, 1]
A1, A2 = [0, 1, 2, 0, 1, 2], np.array([2, 2, 0, 1, 0, 1], dtype=np.int32)
KERNOPS = {"wstep": 40, "qpx": 2, "npixFF": 8, "npixKern": 5}


def uvw_specs(u, v, w, m, form, ncomp):
    """(the p / uvw argument, the specs of its u, v[, w] pointers and the stride) for the tuple and the (n, 3) form"""
    if form == "tuple":
        return (u, v, w), [Arr(u, f64), Arr(v, f64), Arr(w, f64)][:ncomp], 1
    flat = np.array(m, dtype=f64).ravel()  # row-major (n, 3): u at 0, v at 1, w at 2, element stride 3
    return m, [Arr(flat, f64), Arr(flat[1:], f64), Arr(flat[2:], f64)][:ncomp], 3


# ---- the gridders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tuple", "matrix"])
def test_grid_convgrid_convgrid2_degrid2(rig, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    p, (su, sv), st = uvw_specs(u, v, w, m, form, 2)
    if form == "tuple":
        p = (u, v, None)  # the gridders never touch the third component
    a = cplx(8, 12, dtype=c128)
    vis = strided_vis()
    assert run(lambda: ctx.grid(a, p, vis), "gridhip_grid", 8, 12, Same(a), N, su, sv, st, Arr(vis, c128)) is a

    gcf1 = cplx(2, 2, 3, 5)
    assert run(lambda: ctx.convgrid(gcf1, a, p, vis), "gridhip_convgrid", 8, 12, Same(a), N, 2, 3, 5, Arr(gcf1, c128),
               su, sv, st, Arr(vis, c128)) is a

    gcf = cplx(4, 2, 2, 3, 5)[::2]  # complex64 and non-contiguous, W = 2
    spec = [8, 12, Same(a), N, 2, 2, 3, 5, Arr(gcf, c128), su, sv, st, Arr(WBIN, i64)]
    assert run(lambda: ctx.convgrid2(gcf, a, p, WBIN, vis), "gridhip_convgrid2", *spec, Arr(vis, c128)) is a
    # wbin may be NULL in the ABI
    spec[-1] = None
    run(lambda: ctx.convgrid2(gcf, a, p, None, vis), "gridhip_convgrid2", *spec, Arr(vis, c128))
    spec[-1] = Arr(WBIN, i64)

    o = Out(c128, N)
    got = run(lambda: ctx.degrid2(gcf, a, p, np.array(WBIN, dtype=np.int16)), "gridhip_degrid2", *spec, o)
    assert o.returned(got, (N,))
    mine = np.zeros(N, dtype=c128)
    assert run(lambda: ctx.degrid2(gcf, a, p, WBIN, mine), "gridhip_degrid2", *spec, Same(mine)) is mine
    assert run(lambda: ctx.degrid2(gcf, a, p, WBIN, out=mine), "gridhip_degrid2", *spec, Same(mine)) is mine


@pytest.mark.parametrize("form", ["tuple", "matrix"])
def test_convgrid4_degrid4(rig, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    p, (su, sv), st = uvw_specs(u, v, w, m, form, 2)
    a = cplx(8, 12, dtype=c128)
    vis = strided_vis()
    wk, ak = cplx(2, 2, 2, 5, 5), cplx(6, 5, 5)[::2]  # W = 2, Q = 2, S = 5, A = 3
    spec = [8, 12, Same(a), N, 2, 2, 5, 3, Arr(wk, c128), Arr(ak, c128), su, sv, st, Arr(WBIN, i64), Arr(A1, i64),
            Arr(A2, i64)]
    assert run(lambda: ctx.convgrid4(wk, ak, a, p, (WBIN, A1, A2), vis), "gridhip_awgrid", *spec, Arr(vis, c128)) is a
    assert run(lambda: ctx.convgrid3(wk, ak, a, p, [WBIN, A1, A2], vis), "gridhip_awgrid", *spec, Arr(vis, c128)) is a
    o = Out(c128, N)
    assert o.returned(run(lambda: ctx.degrid4(wk, ak, a, p, (WBIN, A1, A2)), "gridhip_awdegrid", *spec, o), (N,))
    mine = np.zeros(N, dtype=c128)
    assert run(lambda: ctx.degrid4(wk, ak, a, p, (WBIN, A1, A2), out=mine), "gridhip_awdegrid", *spec, Same(mine)) is mine


# ---- the imaging functions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tuple", "matrix"])
def test_imaging_functions(rig, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    uvw, (su, sv, sw), st = uvw_specs(u, v, w, m, form, 3)
    vis = strided_vis()
    svis = Arr(vis, c128)

    o = Out(c128, NPIX * NPIX)
    g = run(lambda: ctx.simple_imaging(THETA, LAM, uvw, None, vis), "gridhip_simple_imaging", THETA, LAM, N, su, sv, st,
            svis, o)
    assert o.returned(g, (NPIX, NPIX))

    kv = cplx(2, 2, 3, 5)
    g = run(lambda: ctx.conv_imaging(kv, THETA, LAM, uvw, None, vis), "gridhip_conv_imaging", 2, 3, 5, Arr(kv, c128),
            THETA, LAM, N, su, sv, st, svis, o)
    assert o.returned(g, (NPIX, NPIX))

    g = run(lambda: ctx.w_cache_imaging(KERNOPS, THETA, LAM, uvw, None, vis), "gridhip_w_cache_imaging", 40, 2, 8, 5,
            THETA, LAM, N, su, sv, sw, st, svis, o)
    assert o.returned(g, (NPIX, NPIX))
    # wstep absent or 0: the reference's default of 2000
    for ko in ({"qpx": 2, "npixFF": 8, "npixKern": 5}, dict(KERNOPS, wstep=0), dict(KERNOPS, wstep=None)):
        run(lambda: ctx.w_cache_imaging(ko, THETA, LAM, uvw, None, vis), "gridhip_w_cache_imaging", 2000, 2, 8, 5,
            THETA, LAM, N, su, sv, sw, st, svis, o)

    wk, wv, ak = cplx(2, 2, 2, 5, 5), [-10.0, 30.0], cplx(3, 5, 5)
    tables = [2, 2, 5, 3, Arr(wk, c128), Arr(wv, f64), Arr(ak, c128)]
    for method in (ctx.aw_imaging, ctx.aw_imagingOld):
        g = run(lambda: method(THETA, LAM, wk, wv, ak, uvw, (A1, A2, None, None), vis), "gridhip_aw_imaging", THETA,
                LAM, *tables, N, su, sv, sw, st, Arr(A1, i64), Arr(A2, i64), svis, o)
        assert o.returned(g, (NPIX, NPIX))


def imaging_functions():
    kv = cplx(2, 2, 3, 5)
    wk, wv, ak = cplx(2, 2, 2, 5, 5), np.array([-10, 30], dtype=np.float32), cplx(6, 5, 5)[::2]
    return {"simple": (("simple",), [0, 0, 0, 0, 0, 0, None]),
            "conv": (("conv", kv), [1, 0, 2, 0, 3, 5, Arr(kv, c128)]),
            "w_cache": (("w_cache", KERNOPS), [2, 40, 2, 8, 5, 5, None]),
            "w_cache_default": (("w_cache", {"qpx": 2, "npixFF": 8, "npixKern": 5}), [2, 2000, 2, 8, 5, 5, None]),
            "aw": (("aw", wk, wv, ak), [2, 2, 5, 3, Arr(wk, c128), Arr(wv, f64), Arr(ak, c128)])}


@pytest.mark.parametrize("form", ["tuple", "matrix"])
@pytest.mark.parametrize("kind", ["simple", "conv", "w_cache", "w_cache_default", "aw"])
def test_do_imaging(rig, kind, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    uvw, (su, sv, sw), st = uvw_specs(u, v, w, m, form, 3)
    vis = strided_vis()
    imgfn, head = imaging_functions()[kind]
    oi, op, pm = Out(f64, NPIX * NPIX), Out(f64, NPIX * NPIX), Ref(C.c_double, 2.5)
    op.fill = op.fill * 3
    if kind == "aw":
        spec = [THETA, LAM, *head, N, su, sv, sw, st, Arr(A1, i64), Arr(A2, i64), Arr(vis, c128), oi, op, pm]
        name = "gridhip_do_imaging_aw"
    else:
        spec = [*head, THETA, LAM, N, su, sv, sw, st, Arr(vis, c128), oi, op, pm]
        name = "gridhip_do_imaging"
    img, psf, pmax = run(lambda: ctx.do_imaging(THETA, LAM, uvw, A1, A2, None, None, vis, imgfn), name, *spec)
    assert oi.returned(img, (NPIX, NPIX)) and op.returned(psf, (NPIX, NPIX)) and pmax == 2.5 and type(pmax) is float


@pytest.mark.parametrize("form", ["tuple", "matrix"])
def test_aw_gridding(rig, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    uvw, (su, sv, sw), st = uvw_specs(u, v, w, m, form, 3)
    vis = strided_vis()
    (_, wk, wv, ak), tables = imaging_functions()["aw"]
    o = Out(f64, NPIX * NPIX)
    img, mx = run(lambda: ctx.aw_gridding(THETA, LAM, 1.5e8, wk, wv, ak, uvw, A1, A2, vis), "gridhip_aw_gridding", THETA,
                  LAM, 1.5e8, *tables, N, su, sv, sw, st, Arr(A1, i64), Arr(A2, i64), Arr(vis, c128), o,
                  Ref(C.c_double, 7.0))
    assert o.returned(img, (NPIX, NPIX)) and mx == 7.0


@pytest.mark.parametrize("form", ["tuple", "matrix"])
@pytest.mark.parametrize("kind", ["simple", "conv", "w_cache", "w_cache_default", "aw"])
def test_predict(rig, kind, form):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    uvw, (su, sv, sw), st = uvw_specs(u, v, w, m, form, 3)
    imgfn, head = imaging_functions()[kind]
    model = np.arange(2 * NPIX * NPIX, dtype=np.float32).reshape(NPIX, 2 * NPIX)[:, ::2]  # float32, non-contiguous
    smodel = Arr(model, f64)
    vsub = strided_vis()
    mine = np.zeros(N, dtype=c128)
    inplace = cplx(N, dtype=c128)
    for kw, ssub, sout in (({}, None, Out(c128, N)),
                           ({"vis_sub": vsub}, Arr(vsub, c128), Out(c128, N)),
                           ({"out": mine}, None, Same(mine)),
                           ({"vis_sub": list(vsub), "out": mine}, Arr(vsub, c128), Same(mine)),
                           ({"vis_sub": inplace, "out": inplace}, Same(inplace), Same(inplace))):
        if kind == "aw":
            spec = [THETA, LAM, *head, smodel, N, su, sv, sw, st, Arr(A1, i64), Arr(A2, i64), ssub, sout]
            name = "gridhip_predict_aw"
        else:
            spec = [*head, THETA, LAM, smodel, N, su, sv, sw, st, ssub, sout]
            name = "gridhip_predict"
        got = run(lambda: ctx.predict(THETA, LAM, uvw, model, imgfn, a1=A1, a2=A2, **kw), name, *spec)
        if "out" in kw:
            assert got is kw["out"]
        else:
            assert sout.returned(got, (N,))


# ---- callers either side of the gridder ------------------------------------------------------------------------------
def test_helpers(rig):
    ctx, rec, run = rig
    u, v, w, m = awkward()
    vis = strided_vis()

    o = Out(i64, N)
    wb, mn, npl = run(lambda: ctx.wbins(w, 40.0), "gridhip_wbins", N, Arr(w, f64), 40, o, Ref(C.c_int64, -3),
                      Ref(C.c_int64, 9))
    assert o.returned(wb, (N,)) and (mn, npl) == (-3, 9)

    ws = np.array([-1, 0, 2], dtype=np.float32)
    got = run(lambda: ctx.findClosest(ws, w), "gridhip_find_closest", 3, Arr(ws, f64), N, Arr(w, f64), o)
    assert o.returned(got, (N,))
    o1 = Out(i64, 1)
    got = run(lambda: ctx.findClosest(list(ws), 1.25), "gridhip_find_closest", 3, Arr(ws, f64), 1, Arr([1.25], f64), o1)
    assert o1.returned(got, (1,))

    # mirror_uvw, doweight and make_grid_hermitian work on copies: right-form inputs too are not handed over
    ur, vr, wr = (np.array(x, dtype=f64) for x in (u, v, w))
    visr = np.array(vis, dtype=c128)
    (mu, mv, mw), mvis = run(lambda: ctx.mirror_uvw((ur, vr, wr), visr), "gridhip_mirror_uvw", N, Copy(ur, f64),
                             Copy(vr, f64), Copy(wr, f64), Copy(visr, c128))
    assert all(np.array_equal(x, y) and x.dtype == f64 for x, y in ((mu, ur), (mv, vr), (mw, wr)))
    assert np.array_equal(mvis, visr) and mvis.dtype == c128
    run(lambda: ctx.mirror_uvw((u, v, w), vis), "gridhip_mirror_uvw", N, Arr(u, f64), Arr(v, f64), Arr(w, f64),
        Arr(vis, c128))

    got = run(lambda: ctx.doweight(THETA, LAM, (ur, v, None), visr), "gridhip_doweight", THETA, LAM, N, Same(ur),
              Arr(v, f64), Copy(visr, c128))
    assert np.array_equal(got, visr) and got is not visr

    g = cplx(5, 5, dtype=c128)
    got = run(lambda: ctx.make_grid_hermitian(g), "gridhip_make_grid_hermitian", 5, Copy(g, c128))
    assert np.array_equal(got, g) and got is not g
    gt = cplx(5, 5).T
    run(lambda: ctx.make_grid_hermitian(gt), "gridhip_make_grid_hermitian", 5, Arr(gt, c128))

    img = cplx(2 * NPIX, NPIX)[::2]
    of = Out(c128, NPIX * NPIX)
    for method, inverse in ((ctx.fft, 0), (ctx.ifft, 1)):
        got = run(lambda: method(img), "gridhip_fft2_centered", NPIX, Arr(img, c128), of, inverse)
        assert of.returned(got, (NPIX, NPIX))
    right = cplx(NPIX, NPIX, dtype=c128)
    run(lambda: ctx.fft(right), "gridhip_fft2_centered", NPIX, Same(right), of, 0)

    ok = Out(c128, 2 * 2 * 5 * 5)
    got = run(lambda: ctx.w_kernel(THETA, 100, 8, 5, 2), "gridhip_w_kernel", THETA, 100.0, 8, 5, 2, ok)
    assert ok.returned(got, (2, 2, 5, 5))

    assert ctx.image_size(THETA, LAM) == NPIX and ctx.image_size(0.1, 25) == 2  # round half to even, as Prelude round


def test_comm_convgrid2(rig):
    ctx, rec, run = rig
    from gridhip.distributed import Comm
    h = C.c_void_p(0xFACE)
    comm = Comm(h, rec)
    u, v, w, m = awkward()
    a = cplx(8, 12, dtype=c128)
    vis = strided_vis()
    gcf = cplx(4, 2, 2, 3, 5)[::2]
    spec = [8, 12, Same(a), N, 2, 2, 3, 5, Arr(gcf, c128), Arr(u, f64), Arr(v, f64), 1]
    assert run(lambda: comm.convgrid2(gcf, a, (u, v, None), WBIN, vis), "gridhip_comm_convgrid2", *spec,
               Arr(WBIN, i64), Arr(vis, c128), handle=h) is a
    run(lambda: comm.convgrid2(gcf, a, (u, v, None), None, vis), "gridhip_comm_convgrid2", *spec, None,
        Arr(vis, c128), handle=h)
    with pytest.raises(AssertionError):
        comm.convgrid2(gcf, a.T, (u, v, None), WBIN, vis)
    comm._h = None


# ---- arguments already in the right form go by their own address -----------------------------------------------------
@pytest.mark.parametrize("form", ["tuple", "matrix"])
def test_right_form_is_not_copied(rig, form):
    ctx, rec, run = rig
    u, v, w, m = (np.array(x, dtype=f64) for x in awkward())
    m = np.ascontiguousarray(m)
    if form == "tuple":
        uvw, (su, sv, sw), st = (u, v, w), (Same(u), Same(v), Same(w)), 1
    else:
        uvw, (su, sv, sw), st = m, (Same(m), Same(m, 8), Same(m, 16)), 3
    a = cplx(8, 12, dtype=c128)
    vis, out = cplx(N, dtype=c128), np.zeros(N, dtype=c128)
    wb, a1, a2 = (np.array(x, dtype=i64) for x in (WBIN, A1, A2))
    gcf, kv = cplx(2, 2, 2, 3, 5, dtype=c128), cplx(2, 2, 3, 5, dtype=c128)
    wk, wv, ak = cplx(2, 2, 2, 5, 5, dtype=c128), np.array([-10.0, 30.0]), cplx(3, 5, 5, dtype=c128)
    model = np.arange(NPIX * NPIX, dtype=f64).reshape(NPIX, NPIX)
    tables = [2, 2, 5, 3, Same(wk), Same(wv), Same(ak)]
    oi, pm = Out(f64, NPIX * NPIX), Ref(C.c_double, 1.0)

    run(lambda: ctx.grid(a, uvw, vis), "gridhip_grid", 8, 12, Same(a), N, su, sv, st, Same(vis))
    run(lambda: ctx.convgrid(kv, a, uvw, vis), "gridhip_convgrid", 8, 12, Same(a), N, 2, 3, 5, Same(kv), su, sv, st,
        Same(vis))
    run(lambda: ctx.convgrid2(gcf, a, uvw, wb, vis), "gridhip_convgrid2", 8, 12, Same(a), N, 2, 2, 3, 5, Same(gcf), su,
        sv, st, Same(wb), Same(vis))
    run(lambda: ctx.degrid2(gcf, a, uvw, wb, out), "gridhip_degrid2", 8, 12, Same(a), N, 2, 2, 3, 5, Same(gcf), su, sv,
        st, Same(wb), Same(out))
    aw = [8, 12, Same(a), N, 2, 2, 5, 3, Same(wk), Same(ak), su, sv, st, Same(wb), Same(a1), Same(a2)]
    run(lambda: ctx.convgrid4(wk, ak, a, uvw, (wb, a1, a2), vis), "gridhip_awgrid", *aw, Same(vis))
    run(lambda: ctx.degrid4(wk, ak, a, uvw, (wb, a1, a2), out), "gridhip_awdegrid", *aw, Same(out))
    run(lambda: ctx.simple_imaging(THETA, LAM, uvw, None, vis), "gridhip_simple_imaging", THETA, LAM, N, su, sv, st,
        Same(vis), Out(c128, NPIX * NPIX))
    run(lambda: ctx.conv_imaging(kv, THETA, LAM, uvw, None, vis), "gridhip_conv_imaging", 2, 3, 5, Same(kv), THETA,
        LAM, N, su, sv, st, Same(vis), Out(c128, NPIX * NPIX))
    run(lambda: ctx.w_cache_imaging(KERNOPS, THETA, LAM, uvw, None, vis), "gridhip_w_cache_imaging", 40, 2, 8, 5, THETA,
        LAM, N, su, sv, sw, st, Same(vis), Out(c128, NPIX * NPIX))
    run(lambda: ctx.aw_imaging(THETA, LAM, wk, wv, ak, uvw, (a1, a2), vis), "gridhip_aw_imaging", THETA, LAM, *tables,
        N, su, sv, sw, st, Same(a1), Same(a2), Same(vis), Out(c128, NPIX * NPIX))
    run(lambda: ctx.do_imaging(THETA, LAM, uvw, a1, a2, None, None, vis, ("conv", kv)), "gridhip_do_imaging", 1, 0, 2,
        0, 3, 5, Same(kv), THETA, LAM, N, su, sv, sw, st, Same(vis), oi, oi, pm)
    run(lambda: ctx.do_imaging(THETA, LAM, uvw, a1, a2, None, None, vis, ("aw", wk, wv, ak)), "gridhip_do_imaging_aw",
        THETA, LAM, *tables, N, su, sv, sw, st, Same(a1), Same(a2), Same(vis), oi, oi, pm)
    run(lambda: ctx.aw_gridding(THETA, LAM, 1e8, wk, wv, ak, uvw, a1, a2, vis), "gridhip_aw_gridding", THETA, LAM, 1e8,
        *tables, N, su, sv, sw, st, Same(a1), Same(a2), Same(vis), oi, pm)
    run(lambda: ctx.predict(THETA, LAM, uvw, model, ("conv", kv), vis_sub=vis, out=out), "gridhip_predict", 1, 0, 2, 0,
        3, 5, Same(kv), THETA, LAM, Same(model), N, su, sv, sw, st, Same(vis), Same(out))
    run(lambda: ctx.predict(THETA, LAM, uvw, model, ("aw", wk, wv, ak), a1=a1, a2=a2, vis_sub=vis, out=out),
        "gridhip_predict_aw", THETA, LAM, *tables, Same(model), N, su, sv, sw, st, Same(a1), Same(a2), Same(vis),
        Same(out))
    run(lambda: ctx.wbins(w, 40), "gridhip_wbins", N, Same(w), 40, Out(i64, N), Ref(C.c_int64, 0), Ref(C.c_int64, 1))
    run(lambda: ctx.findClosest(wv, w), "gridhip_find_closest", 2, Same(wv), N, Same(w), Out(i64, N))


# ---- refusals come before any call -----------------------------------------------------------------------------------
def test_refusals_are_raised_before_any_call(rig):
    ctx, rec, run = rig
    u, v, w, m = (np.array(x, dtype=f64) for x in awkward())
    vis = cplx(N, dtype=c128)
    model = np.zeros((NPIX, NPIX))
    a = cplx(8, 12, dtype=c128)
    gcf = cplx(2, 2, 2, 3, 5, dtype=c128)
    bad = [
        lambda: ctx.do_imaging(THETA, LAM, m, A1, A2, None, None, vis, ("a_projection",)),
        lambda: ctx.predict(THETA, LAM, m, model, ("a_projection",)),
        lambda: ctx.predict(THETA, LAM, m, np.zeros((NPIX, NPIX + 1)), ("simple",)),         # model shape
        lambda: ctx.predict(THETA, LAM, m, np.zeros(NPIX * NPIX), ("simple",)),
        lambda: ctx.predict(THETA, LAM, m, model, ("simple",), out=np.zeros(N, dtype=np.complex64)),  # out dtype
        lambda: ctx.predict(THETA, LAM, m, model, ("simple",), out=np.zeros(2 * N, dtype=c128)[::2]),  # not contiguous
        lambda: ctx.predict(THETA, LAM, m, model, ("simple",), out=[0j] * N),                # not an array
        lambda: ctx.predict(THETA, LAM, m, model, ("simple",), out=np.zeros(N + 1, dtype=c128)),      # lengths
        lambda: ctx.predict(THETA, LAM, (u, v, w), model, ("simple",), vis_sub=vis[:-1]),
        lambda: ctx.predict(THETA, LAM, m, model, ("aw", gcf, [0.0, 1.0], gcf[0, 0]), a1=A1, a2=A2, vis_sub=vis[:-1]),
        lambda: ctx.grid(a.astype(np.complex64), (u, v, None), vis),                         # the grid is written in place
        lambda: ctx.convgrid2(gcf, a.T, (u, v, None), WBIN, vis),
        lambda: ctx.degrid2(gcf, [[0j] * 4] * 4, m, WBIN),
        lambda: ctx.convgrid2(gcf, a, m[:, :2], WBIN, vis),                                   # neither a tuple nor (n, 3)
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert rec.calls == [], f"refusal {k} came after {rec.calls}"
