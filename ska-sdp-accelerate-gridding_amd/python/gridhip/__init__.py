"""gridhip — Python binding of libgridhip.so, the MI355X-native w-projection gridder.

The module mirrors the gridder interface of the reference's src/Gridding.hs — same names,
argument order and meaning:

    grid      a p v            (src/Gridding.hs:95-98)
    convgrid  gcf a p v        (src/Gridding.hs:153-157)
    convgrid2 gcf a p wbin v   (src/Gridding.hs:199-204)
    degrid2   gcf a p wbin     (the gather twin; absent from the reference)
    convgrid4 wkerns akerns a p index v   (src/Gridding.hs:318-324; convgrid3 gives the same grid)
    degrid4   wkerns akerns a p index     (the gather twin of convgrid4; absent from the reference)

`a` is the destination grid (complex128, [H, W], ACCUMULATED INTO and returned), `p` the
baselines already scaled to (-.5, .5) — a (u, v, w) tuple of float64 arrays or an (n, 3)
array — `v` the visibilities (complex128).  numpy arguments take the synchronous host path of
the C ABI; torch CUDA tensors take the asynchronous device path on torch's current stream.
Every argument of either kind is marshalled by _marshal.py.

There is no CPU fallback: importing works anywhere the library is built, computing needs a
gfx950 GPU.
"""
import ctypes as C

from . import _lib
from ._lib import GridHipError, LIB_PATH  # noqa: F401
from ._marshal import (HOST, Handle, aw_kernels, aw_tables, backend, baselines, beam_support, clean_scalars, device,
                       auto_args, image_of, imaging_function, in_place, is_torch, mask_of, scale_list)
from ._marshal import gain_stream, result_array, solve_args, stream_array
from ._marshal import direction_mask, model_rows
from ._marshal import jones_array, stokes_args
from ._marshal import flag_outputs, flag_scalars, flag_stream
from ._marshal import cube_arrays, sumthreshold_scalars
from ._marshal import COMP_DOUBLES, component_count, component_list, model_planes
from ._marshal import automask_args, mask_in_place, source_args
from ._marshal import group_ids, rotation as _rotation
from ._marshal import weighting as _weighting
from ._marshal import mosaic_args
from ._marshal import idg_options, idg_trusted, stack_options, wstack_options
from ._marshal import JOINT_MAX_PLANES, joint_search, psf_planes
from ._marshal import RM_MAPS, rm_clean_scalars, rm_cube, rm_images, rm_table_args, rm_table_doubles, rm_table_of
from ._marshal import contsub_args
from ._marshal import FRINGE_MAX_DELAYS, FRINGE_MAX_RATES, FRINGE_PEAK, fringe_cube, fringe_intervals, fringe_sol
from ._marshal import fringe_solve_scalars, fringe_table_args, fringe_table_doubles, fringe_table_of
from ._marshal import TEC_HEAD, TEC_KAPPA, TEC_MAX_CELLS, TEC_MAX_DELAYS, TEC_PEAK, tec_table_args, tec_table_doubles, tec_table_of

__all__ = ["Context", "default_context", "grid", "convgrid", "convgrid2", "degrid2", "GridHipError", "components", "flag_groups", "ddcal_lds_antennas", "jonescal_lds_antennas",
           "rotation_to", "rotation_radec", "average_groups", "facet_grid", "joint_deconvolve", "sumthreshold_tile",
           "waterfall_layout", "rm_tile", "faraday_grid", "contsub_tile", "channel_coordinate",
           "fringe_tile", "fringe_grid", "tec_tile", "tec_grid", "tec_clock", "tec_coordinates", "TEC_KAPPA", "idg_trusted",
           "SOURCE_BLENDED"]

SOURCE_BLENDED = 8  # flag bit 3 of a find_sources info row: the row's island was split into several rows (deblend > 0)


def _deblended(ctx, deblend, call):
    """call() with the option "sources_deblend" at `deblend`, put back afterwards; 0 leaves the option alone"""
    deblend = int(deblend)
    if deblend < 0:
        raise ValueError("deblend must be >= 0")
    if deblend == 0:
        return call()
    before = ctx.get_option("sources_deblend")
    ctx.set_option("sources_deblend", deblend)
    try:
        return call()
    finally:
        ctx.set_option("sources_deblend", before)


class Context(Handle):
    """One device + one stream (gridhip_ctx).  Not thread-safe."""
    _destroy = "gridhip_destroy"
    _ctx = property(lambda self: self)

    def __init__(self, device=0):
        self._lib, self._h = _lib.load(), None
        h = C.c_void_p()
        self._check(self._lib.gridhip_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    # -- plumbing ---------------------------------------------------------------------------
    def _error(self, rc):
        return (self._h and self._lib.gridhip_last_error(self._h).decode()) or self._lib.gridhip_strerror(rc).decode()

    def set_option(self, key, value):
        self._check(self._lib.gridhip_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int64()
        self._check(self._lib.gridhip_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def set_stream(self, stream_ptr):
        """Enqueue on this hipStream_t; 0/None is HIP's default (null) stream."""
        self._check(self._lib.gridhip_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def reset_stream(self):
        self._check(self._lib.gridhip_reset_stream(self._h))

    def synchronize(self):
        self._check(self._lib.gridhip_synchronize(self._h))

    def enable_timing(self, on=True):
        self._check(self._lib.gridhip_enable_timing(self._h, int(bool(on))))

    def last_timing(self):
        """(total_ms, prepass_ms, kernel_ms) of the last device call, from HIP events on the stream."""
        t, p, k = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.gridhip_last_timing(self._h, C.byref(t), C.byref(p), C.byref(k)))
        return t.value, p.value, k.value

    def timing(self, back=0):
        """(total_ms, prepass_ms, kernel_ms) of the timed device call `back` calls before the last one."""
        t, p, k = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.gridhip_timing(self._h, int(back), C.byref(t), C.byref(p), C.byref(k)))
        return t.value, p.value, k.value

    def last_dropped(self):
        d = C.c_int64()
        self._check(self._lib.gridhip_last_dropped(self._h, C.byref(d)))
        return d.value

    def _use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ptr(x):
        return None if x is None else backend(x).ptr(x)

    # -- the gridders ---------------------------------------------------------------------------
    @staticmethod
    def _gridder(a, p, vis, write=False):
        """What every gridder starts with: the back end of the grid `a`, u, v and their stride from `p`, n, and the
        visibilities: read (scatter), or written (gather: `vis` is the caller's output, None for a new one)."""
        be = backend(a)
        u, v, stride = baselines(be, p, 2)
        if not be.ok(a, be.c128):
            raise be.bad_grid(f"grid must be {be.form} (it is accumulated in place)")
        n = int(u.shape[0])
        if not write:
            vis = be.cv(vis, be.c128)
        elif vis is None:
            vis = be.empty(n, be.c128, a)
        return be, u, v, stride, n, vis

    def grid(self, a, p, v):
        """src/Gridding.hs:95-112"""
        be, pu, pv, stride, n, vis = self._gridder(a, p, v)
        self._call(be, "grid", a.shape[0], a.shape[1], a, n, pu, pv, stride, vis)
        return a

    def convgrid(self, gcf, a, p, v):
        """src/Gridding.hs:153-197 ; gcf [Q,Q,gh,gw]"""
        be, pu, pv, stride, n, vis = self._gridder(a, p, v)
        gcf = be.cv(gcf, be.c128)
        Q, Q2, gh, gw = gcf.shape
        assert Q == Q2
        self._call(be, "convgrid", a.shape[0], a.shape[1], a, n, Q, gh, gw, gcf, pu, pv, stride, vis)
        return a

    def _grid2(self, name, gcf, a, p, wbin, vis, write):
        """convgrid2 and degrid2: one argument list, whose last entry is read or written"""
        be, pu, pv, stride, n, vis = self._gridder(a, p, vis, write)
        gcf = be.cv(gcf, be.c128)
        W, Q, Q2, gh, gw = gcf.shape
        assert Q == Q2
        self._call(be, name, a.shape[0], a.shape[1], a, n, W, Q, gh, gw, gcf, pu, pv, stride, be.cv(wbin, be.i64), vis)
        return vis

    def convgrid2(self, gcf, a, p, wbin, v):
        """src/Gridding.hs:199-244 ; gcf [W,Q,Q,gh,gw]"""
        self._grid2("convgrid2", gcf, a, p, wbin, v, False)
        return a

    def degrid2(self, gcf, a, p, wbin, out=None):
        """Gather with convgrid2's coordinates: out[k] = sum_ij gcf[wbin,yf,xf,i,j] * a[y0+i,x0+j]."""
        return self._grid2("degrid2", gcf, a, p, wbin, out, True)

    def plan(self, grid_shape, gcf_shape, p, wbin):
        """Bin the baselines `p` (torch cuda tensors) once for an [H, W] grid and a [W,Q,Q,gh,gw] kernel
        table; returns a Plan whose grid()/degrid() skip the pre-pass."""
        be = device()
        u, v, stride = baselines(be, p, 2)
        W, Q, _, gh, gw = gcf_shape
        n, h = int(u.shape[0]), C.c_void_p()
        self._call(be, "plan_create", grid_shape[0], grid_shape[1], n, W, Q, gh, gw, u, v, stride, be.cv(wbin, be.i64),
                   C.byref(h))
        return Plan(self, h, n, tuple(grid_shape), tuple(gcf_shape))

    def _grid4(self, name, wkerns, akerns, a, p, index, vis, write):
        """convgrid4 and degrid4, as _grid2"""
        be, pu, pv, stride, n, vis = self._gridder(a, p, vis, write)
        tables, idx = aw_kernels(be, wkerns, akerns, index)
        self._call(be, name, a.shape[0], a.shape[1], a, n, *tables, pu, pv, stride, *idx, vis)
        return vis

    def convgrid4(self, wkerns, akerns, a, p, index, v):
        """src/Gridding.hs:318-396 ; index = (wbin, a1, a2) arrays.  convgrid3 (:246-317) gives the same grid."""
        self._grid4("awgrid", wkerns, akerns, a, p, index, v, False)
        return a

    convgrid3 = convgrid4

    def degrid4(self, wkerns, akerns, a, p, index, out=None):
        """The gather twin of convgrid4 (gridhip_awdegrid): out[k] = sum_ij awkern_k[i,j] * a[y0+i, x0+j] with the
        kernel convgrid4 scatters, awkern_k = conj(aw_kernel_fn2(yf, xf, wkerns[wbin], akerns[a1], akerns[a2])).
        index = (wbin, a1, a2); out of range indices predict 0 (counted in last_dropped).  Returns out (overwritten)."""
        return self._grid4("awdegrid", wkerns, akerns, a, p, index, out, True)

    def aw_plan(self, grid_shape, wkerns, akerns, p, index):
        """Key, build and bin the baselines `p` (torch cuda tensors) once for an [H, W] grid (gridhip_aw_plan).  The plan
        keeps the kernels built from wkerns / akerns: the arguments may be freed or changed afterwards.  Returns an
        AwPlan whose grid() / degrid() run the tile kernel only."""
        be = device()
        u, v, stride = baselines(be, p, 2)
        tables, idx = aw_kernels(be, wkerns, akerns, index)
        n, h = int(u.shape[0]), C.c_void_p()
        self._call(be, "aw_plan_create", grid_shape[0], grid_shape[1], n, *tables, u, v, stride, *idx, C.byref(h))
        return AwPlan(self, h, n, tuple(grid_shape))

    def aw_stats(self, S=15):
        """What the last convgrid4 did: visibilities keyed, distinct kernels built, the hit rate of the per-key
        de-duplication, the fp64 flops of the kernel builds and (timing enabled) their device time."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.gridhip_aw_last_stats(self._h, C.byref(a), C.byref(b)))
        c = S // 2
        macs = sum(S - abs(y - c) for y in range(S)) ** 2  # complex products of one 'same' S x S convolution (15: 28 561)
        out = {"vis_keyed": a.value, "kernels_built": b.value,
               "hit_rate": 1.0 - b.value / a.value if a.value else 0.0,
               "conv_flops_per_call": 8.0 * macs * b.value}
        try:
            t = self.timing(0)
            out.update(build_ms=t[1], grid_ms=t[2])
        except GridHipError:
            pass
        return out

    # -- callers either side of the gridder (host arrays; src/Gridding.hs names) -----------------
    def image_size(self, theta, lam):
        return int(self._lib.gridhip_image_size(float(theta), int(lam)))

    def wbins(self, w, wstep):
        """w-bin rule of w_cache_imaging (:426-432) -> (wbin, wmin, nplanes)"""
        w = HOST.cv(w, HOST.f64)
        out = HOST.empty(len(w), HOST.i64, w)
        mn, npl = C.c_int64(), C.c_int64()
        self._call(HOST, "wbins", len(w), w, int(wstep), out, C.byref(mn), C.byref(npl))
        return out, mn.value, npl.value

    def findClosest(self, ws, w):
        """:895-907, vectorised over w"""
        ws, w = HOST.cv(ws, HOST.f64), HOST.cv(w, HOST.f64)  # (a scalar w becomes one element)
        out = HOST.empty(len(w), HOST.i64, w)
        self._call(HOST, "find_closest", len(ws), ws, len(w), w, out)
        return out

    def mirror_uvw(self, uvw, vis):
        """:551-562 -> ((u, v, w), vis)"""
        u, v, w = (HOST.cv(x, HOST.f64).copy() for x in uvw)
        vis = HOST.cv(vis, HOST.c128).copy()
        self._call(HOST, "mirror_uvw", len(u), u, v, w, vis)
        return (u, v, w), vis

    def doweight(self, theta, lam, p, v):
        """:564-583 ; p in wavelengths"""
        u, vv = HOST.cv(p[0], HOST.f64), HOST.cv(p[1], HOST.f64)
        vis = HOST.cv(v, HOST.c128).copy()
        self._call(HOST, "doweight", float(theta), int(lam), len(u), u, vv, vis)
        return vis

    def make_grid_hermitian(self, guv):
        """:585-605"""
        g = HOST.cv(guv, HOST.c128).copy()
        self._call(HOST, "make_grid_hermitian", g.shape[0], g)
        return g

    def _fft(self, m, inverse):
        m = HOST.cv(m, HOST.c128)
        out = HOST.empty(m.shape, HOST.c128, m)
        self._call(HOST, "fft2_centered", m.shape[0], m, out, int(inverse))
        return out

    def ifft(self, m):
        """:828-829"""
        return self._fft(m, True)

    def fft(self, m):
        """:815-816 (fftO)"""
        return self._fft(m, False)

    def w_kernel(self, theta, w, npixFF, npixKern, qpx):
        """:610-619 -> [qpx, qpx, npixKern, npixKern]"""
        out = HOST.empty((qpx, qpx, npixKern, npixKern), HOST.c128, None)
        self._call(HOST, "w_kernel", float(theta), float(w), int(npixFF), int(npixKern), int(qpx), out)
        return out

    # -- the imaging functions and their callers ----------------------------------------------------
    def _imaging(self, be, theta, lam, uvw, vis):
        """What every imaging call starts with: (theta, lam), (n, u, v, w, stride), the visibilities, and the shape
        (N, N) of its outputs"""
        N = self.image_size(theta, lam)
        u, v, w, st = baselines(be, uvw, 3)
        vis = be.cv(vis, be.c128)
        return (float(theta), int(lam)), (int(vis.shape[0]), u, v, w, st), vis, (N, N)

    def simple_imaging(self, theta, lam, uvw, src, vis):
        """:84-93 (src is unused by this imaging function, as in the reference)"""
        tl, (n, u, v, _, st), vis, NN = self._imaging(HOST, theta, lam, uvw, vis)
        g = HOST.empty(NN, HOST.c128, vis)
        self._call(HOST, "simple_imaging", *tl, n, u, v, st, vis, g)
        return g

    def conv_imaging(self, kv, theta, lam, uvw, src, vis):
        """:115-124 ; kv [Q,Q,gh,gw]"""
        tl, (n, u, v, _, st), vis, NN = self._imaging(HOST, theta, lam, uvw, vis)
        g = HOST.empty(NN, HOST.c128, vis)
        _, _, Q, _, gh, gw, kv = imaging_function(HOST, ("conv", kv))
        self._call(HOST, "conv_imaging", Q, gh, gw, kv, *tl, n, u, v, st, vis, g)
        return g

    def w_cache_imaging(self, kernops, theta, lam, uvw, src, vis):
        """:399-449 ; kernops = dict(wstep=, qpx=, npixFF=, npixKern=) as KernelOptions (:30-38).
        torch cuda tensors take the device-resident form (gridhip_w_cache_imaging_dev) and return a cuda tensor."""
        be = backend(vis)
        tl, stream, vis, NN = self._imaging(be, theta, lam, uvw, vis)
        g = be.empty(NN, be.c128, vis)
        _, wstep, qpx, npixFF, side, _, _ = imaging_function(be, ("w_cache", kernops))
        self._call(be, "w_cache_imaging", wstep, qpx, npixFF, side, *tl, *stream, vis, g)
        return g

    def aw_imaging(self, theta, lam, wkernels, wbins, akernels, uvw, src, vis):
        """src/Gridding.hs:452-478 (aw_imagingOld :480-506 gives the same grid); src = (a1, a2, t, f).
        torch cuda tensors take the device-resident form (gridhip_aw_imaging_dev) and return a cuda tensor."""
        be = backend(vis)
        tl, stream, vis, NN = self._imaging(be, theta, lam, uvw, vis)
        g = be.empty(NN, be.c128, vis)
        tables, a1, a2 = aw_tables(be, wkernels, wbins, akernels, src[0], src[1])
        self._call(be, "aw_imaging", *tl, *tables, *stream, a1, a2, vis, g)
        return g

    aw_imagingOld = aw_imaging

    def do_imaging(self, theta, lam, uvw, a1, a2, t, f, vis, imgfn):
        """:509-549 -> (image, psf, pmax).  imgfn = ("simple",) | ("conv", kv) | ("w_cache", kernops) |
        ("aw", wkernels, wbins, akernels) | ("wstack", dict(wstep=, planes=, qpx=, npixFF=, npixKern=)) - w-stacking, whose
        image is 2 Re D instead of the Hermitian fill (include/gridhip.h, "w-stacking") | ("idg", dict(wstep=, planes=,
        subgrid=, margin=)) - the same stack with image-domain layers: every visibility with its exact w on subgrids of
        `subgrid` (16, 24, 32) cells with a margin of `margin` (even, 4 .. subgrid / 2), no kernel table; image and psf are
        exactly 0 outside the trusted region [idg_trusted(N), idg_trusted(N)]; a1, a2 feed the antenna indices of "aw" (not swapped by the mirror), t, f
        (src) are accepted for signature parity and unused by these imaging functions.
        torch cuda tensors (uvw, vis, and kv / the aw tables and antennas) take the device-resident form
        (gridhip_do_imaging_dev / gridhip_do_imaging_aw_dev): nothing crosses PCIe, image and psf come back as cuda
        tensors."""
        be = backend(vis)
        tl, stream, vis, NN = self._imaging(be, theta, lam, uvw, vis)
        img, psf, pmax = be.empty(NN, be.f64, vis), be.empty(NN, be.f64, vis), C.c_double()
        if imgfn[0] == "aw":
            tables, a1, a2 = aw_tables(be, imgfn[1], imgfn[2], imgfn[3], a1, a2)
            self._call(be, "do_imaging_aw", *tl, *tables, *stream, a1, a2, vis, img, psf, C.byref(pmax))
        elif imgfn[0] in ("wstack", "idg"):
            self._call(be, "do_imaging_wstack", *stack_options(imgfn), *tl, *stream, vis, img, psf, C.byref(pmax))
        else:
            self._call(be, "do_imaging", *imaging_function(be, imgfn), *tl, *stream, vis, img, psf, C.byref(pmax))
        return img, psf, pmax.value

    def aw_gridding(self, theta, lam, f, wkernels, wbins, akernels, uvw_m, a1, a2, vis):
        """src/ImageDataset.hs:54-77 as one call (gridhip_aw_gridding[_dev]): uvw_m in metres ((n, 3) or a (u, v, w)
        tuple), f in Hz; doweight on the un-mirrored uvw, mirror, aw_imaging, make_grid_hermitian, real . ifft.
        Returns (image, max pixel); torch cuda tensors take the device-resident form and return a cuda image."""
        be = backend(vis)
        tl, stream, vis, NN = self._imaging(be, theta, lam, uvw_m, vis)
        tables, a1, a2 = aw_tables(be, wkernels, wbins, akernels, a1, a2)
        img, mx = be.empty(NN, be.f64, vis), C.c_double()
        self._call(be, "aw_gridding", *tl, float(f), *tables, *stream, a1, a2, vis, img, C.byref(mx))
        return img, mx.value

    def predict(self, theta, lam, uvw, model, imgfn, a1=None, a2=None, vis_sub=None, out=None):
        """Visibilities of a real N x N model image (gridhip_predict[_aw][_dev]): the adjoint of the imaging function
        `imgfn` applied to fft_c(model), or vis_sub minus that (the residual) when vis_sub is given.  imgfn takes
        do_imaging's tuples: ("simple",) | ("conv", kv) | ("w_cache", kernops) | ("aw", wkernels, wbins, akernels), the
        last with the antenna indices a1, a2, | ("wstack", kernops with planes=) | ("idg", dict(wstep=, planes=, subgrid=,
        margin=)), which reads the model inside the trusted region only.  uvw (wavelengths, not mirrored) as the imaging function takes it.
        numpy in gives numpy out; torch cuda tensors take the device form on torch's stream and return a cuda tensor.
        out: the array to write (may be vis_sub itself: an in-place residual); a new one when None."""
        be = backend(model)
        N = self.image_size(theta, lam)
        if tuple(model.shape) != (N, N):
            raise ValueError(f"model must be {N} x {N} (image_size(theta, lam)), not {tuple(model.shape)}")
        u, v, w, st = baselines(be, uvw, 3)
        model, sub, n = be.cv(model, be.f64), be.cv(vis_sub, be.c128), int(u.shape[0])
        if out is None:
            out = be.empty(n, be.c128, model)
        elif not be.ok(out, be.c128):
            raise ValueError(f"out must be {be.form}")
        if len(out) != n or (sub is not None and len(sub) != n):
            raise ValueError("vis_sub and out must hold one value per visibility")
        tl = float(theta), int(lam)
        if imgfn[0] == "aw":
            tables, a1, a2 = aw_tables(be, imgfn[1], imgfn[2], imgfn[3], a1, a2)
            self._call(be, "predict_aw", *tl, *tables, model, n, u, v, w, st, a1, a2, sub, out)
        elif imgfn[0] in ("wstack", "idg"):
            self._call(be, "predict_wstack", *stack_options(imgfn), *tl, model, n, u, v, w, st, sub, out)
        else:
            self._call(be, "predict", *imaging_function(be, imgfn), *tl, model, n, u, v, w, st, sub, out)
        return out

    def image_stats(self, image, mask=None, border=0):
        """Robust statistics of the N x N float64 `image` (gridhip_image_stats[_dev]; include/gridhip.h, "image
        statistics") over the finite cells inside `border` and `mask` (bool or uint8, N x N, None: every cell):
        [n, median, MAD, sigma = 1.4826 MAD, min, max, non-finite cells skipped, 0] - exact order statistics, the same
        bits on every run.  A numpy image takes the synchronous host form; a torch cuda tensor the asynchronous one, and
        the result is a cuda tensor: nothing is read back (stats[3:4] is the `noise` of clean)."""
        be = backend(image)
        shape = tuple(getattr(image, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("image must be N x N")
        image = image_of(be, image, shape, "image")
        mask = mask_of(be, mask, shape)
        stats = be.empty(8, be.f64, image)
        self._call(be, "image_stats", shape[0], image, mask, int(border), stats)
        return stats

    def noise_map(self, image, mask=None, exclude=False, border=0, step=16, half=None, kappa=3.0, nclip=3, min_count=16,
                  mode=None, maps=True, out=None):
        """Local background and noise maps of the N x N float64 `image` (gridhip_noise_map[_dev]; include/gridhip.h,
        "local background and noise maps"): the lower median and 1.4826 MAD of the (2 half + 1)^2 window around every
        node of a mesh `step` cells apart, clipped at `kappa` sigma for up to `nclip` rounds, interpolated onto the
        image.  half=None means min(64, 2 * step).  `mask` (bool or uint8, N x N) names the cells that take part, or with
        exclude=True the cells that do not - a clean mask then keeps its sources out of their own noise estimate.
        mode: None, "subtract" (out = image - background) or "snr" (out = (image - background) / rms); `out` is the
        array to write, which may be `image` itself, a new one when None.  maps=False leaves the two maps out.
        Returns (background, rms, out, nodes, stats): nodes is [4, G, G] = background, rms, cells used, clip rounds per
        node, NaN where a node has fewer than `min_count` cells (and for the rms of a constant patch);
        stats = [G, nodes with a background, nodes with an rms, smallest and largest node rms, non-finite cells of out,
        most rounds, 0].  ctx.image_stats(nodes[1]) gives one typical sigma (it skips the NaNs).  numpy in gives numpy
        out; torch cuda tensors take the asynchronous device form, which reads nothing back and can be captured."""
        be = backend(image)
        shape = tuple(getattr(image, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("image must be N x N")
        modes = {None: 0, "subtract": 1, "snr": 2}
        if mode not in modes:
            raise ValueError('mode must be None, "subtract" or "snr"')
        step = int(step)
        half = min(64, 2 * step) if half is None else int(half)
        G = int(self._lib.gridhip_noise_map_nodes(shape[0], int(border), step))
        if G < 0:
            raise GridHipError(G, "noise_map: N, border or step out of range")
        if out is not None and out is image:
            out = image = in_place(be, image, shape, "image")
        else:
            image = image_of(be, image, shape, "image")
            if mode is None:
                out = None
            elif out is None:
                out = be.empty(shape, be.f64, image)
            else:
                out = in_place(be, out, shape, "out")
        mask = mask_of(be, mask, shape)
        bg, rms = (be.empty(shape, be.f64, image), be.empty(shape, be.f64, image)) if maps else (None, None)
        nodes, stats = be.empty((4, G, G), be.f64, image), be.empty(8, be.f64, image)
        self._call(be, "noise_map", shape[0], image, mask, int(bool(exclude)), int(border), step, half, float(kappa),
                   int(nclip), int(min_count), modes[mode], nodes, bg, rms, out, stats)
        return bg, rms, out, nodes, stats

    def automask_local(self, image, mask=None, border=0, step=16, half=None, kappa=3.0, nclip=3, min_count=16,
                       nsigma=(5, 2.5), min_cells=1, grow=0, absolute=False):
        """automask against the LOCAL noise: noise_map(mode="snr") - with `mask` given, over the cells outside it
        (exclude=True) - and then automask on the S/N image with the fixed levels thr=nsigma, so that nsigma[0] means
        that many local sigma everywhere in the map.  `mask` is updated in place as automask does.  Returns
        (mask, automask's stats, the S/N image, noise_map's stats)."""
        _, _, snr, _, nstats = self.noise_map(image, mask=mask, exclude=mask is not None, border=border, step=step,
                                              half=half, kappa=kappa, nclip=nclip, min_count=min_count, mode="snr",
                                              maps=False)
        mask, astats = self.automask(snr, mask=mask, border=border, absolute=absolute, thr=nsigma, nsigma=(0, 0),
                                     min_cells=min_cells, grow=grow)
        return mask, astats, snr, nstats

    def automask(self, image, mask=None, noise=None, border=0, absolute=False, thr=(0, 0), nsigma=(5, 2.5), peak_frac=0,
                 min_cells=1, grow=0):
        """The clean mask of the N x N float64 `image` (gridhip_automask[_dev]; include/gridhip.h, "auto-masking"): the
        islands above T_hi = max(thr[0], nsigma[0] * sigma, peak_frac * peak) with at least `min_cells` cells
        (8-connected), each extended to the whole island above T_lo = max(thr[1], nsigma[1] * sigma, peak_frac * peak) it
        lies in, grown by `grow` cells, OR-ed into `mask`.  `mask` (uint8 or bool, N x N; zeros when None) is UPDATED IN
        PLACE and returned; bytes that are not 0 stay as they are.  `noise` is sigma: a number, or one element like
        image_stats(...)[3:4]; nsigma=0 takes fixed levels and needs none.  absolute: |image| is thresholded.  Returns
        (mask, stats); stats = [T_hi, T_lo, peak, components above T_hi, of them surviving the prune, components above
        T_lo kept, cells newly set, reason (0; 2: no cell takes part, 3: sigma is NaN - the mask is then untouched)].
        numpy arrays take the synchronous host form; torch cuda tensors the asynchronous one, with stats a cuda tensor:
        nothing is read back.  With cuda tensors pass `noise` as a device element to stay capturable."""
        be = backend(image)
        shape = tuple(getattr(image, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("image must be N x N")
        image = image_of(be, image, shape, "image")
        args = automask_args(be, absolute, thr, nsigma, noise, peak_frac, min_cells, grow, image)
        mask, m8 = mask_in_place(be, mask, shape, image)
        stats = be.empty(8, be.f64, image)
        self._call(be, "automask", shape[0], image, m8, int(border), *args, stats)
        return mask, stats

    def clean(self, image, psf, gain=0.1, threshold=0.0, niter=100, border=0, patch=0, model=None, mask=None,
              nsigma=0.0, noise=None, peak_frac=0.0):
        """Hogbom CLEAN of the N x N float64 `image` with `psf` (gridhip_clean[_dev]; include/gridhip.h,
        "deconvolution"): at most niter components of gain * peak, searched inside `border`, stopping at |peak| <=
        threshold, the PSF subtracted over its whole overlap or (patch > 0) within +-patch cells of the peak.
        `image` is UPDATED IN PLACE and returned as the residual; `model` (zeros when None) is accumulated into and
        returned, so `model, residual, stats = ctx.clean(image, psf, model=model)` is model = model + clean(image, psf).
        stats = [iterations, final peak, its flat index, flux added].  numpy arrays take the synchronous host form;
        torch cuda tensors the asynchronous one on torch's stream, with stats a cuda tensor: nothing is read back.
        With any of `mask` (bool or uint8, N x N: cells that are 0 are never selected), `nsigma` and `noise` (sigma: a
        number, or one element like image_stats(...)[3:4]) or `peak_frac` the call is gridhip_clean_auto[_dev]
        ("masks and noise-based stop levels"): the loop stops at T = max(threshold, nsigma * sigma, peak_frac * |first
        peak|) and stats has four more values, [T, reason, first peak, 0].  With cuda tensors pass `noise` as a device
        element (stats[3:4]): a Python number is uploaded by a host-to-device copy, so the call is then neither
        asynchronous nor capturable into a graph."""
        be = backend(image)
        shape = tuple(getattr(image, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("image must be N x N")
        image = in_place(be, image, shape, "image")
        psf = be.cv(psf, be.f64)
        if tuple(psf.shape) != shape:
            raise ValueError(f"psf must be {shape}, as the image")
        model = in_place(be, model, shape, "model", image)
        auto = auto_args(be, mask, nsigma, noise, peak_frac, shape, image)
        stats = be.empty(8 if auto else 4, be.f64, image)
        if auto:
            self._call(be, "clean_auto", shape[0], psf, image, model, *clean_scalars(gain, threshold, niter, border, patch),
                       *auto, stats)
        else:
            self._call(be, "clean", shape[0], psf, image, model, *clean_scalars(gain, threshold, niter, border, patch),
                       stats)
        return model, image, stats

    def msclean(self, image, psf, scales, bias=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0, model=None,
                mask=None, nsigma=0.0, noise=None, peak_frac=0.0):
        """Multi-scale CLEAN of the N x N float64 `image` with `psf` (gridhip_msclean[_dev]; include/gridhip.h,
        "multi-scale deconvolution"): clean() whose components are tapered paraboloids of the `scales` (in cells,
        increasing from the delta scale 0, at most 6 of them and at most 32 cells), chosen by the largest bias-weighted
        peak.  `scales` and `bias` are host sequences for numpy and torch images alike; bias=None is
        1 - 0.6 a_s / a_max.  `image` is UPDATED IN PLACE and returned as the residual, `model` (zeros when None) is
        accumulated into.  Returns (model, residual, stats); stats = [iterations, final peak, its flat index, the scale
        of the last component (-1: none), flux added, 0, components per scale x 6].  mask, nsigma, noise, peak_frac: as
        for clean (gridhip_msclean_auto[_dev]); the mask constrains component centres, and stats has 16 values.  As
        for clean, a numeric `noise` with cuda tensors is a host-to-device copy and cannot be captured: pass stats[3:4]."""
        be = backend(image)
        shape = tuple(getattr(image, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("image must be N x N")
        image = in_place(be, image, shape, "image")
        psf = be.cv(psf, be.f64)
        if tuple(psf.shape) != shape:
            raise ValueError(f"psf must be {shape}, as the image")
        sc, keep = scale_list(scales, bias)
        model = in_place(be, model, shape, "model", image)
        auto = auto_args(be, mask, nsigma, noise, peak_frac, shape, image)
        stats = be.empty(16 if auto else 12, be.f64, image)
        if auto:
            self._call(be, "msclean_auto", shape[0], psf, image, model, *sc,
                       *clean_scalars(gain, threshold, niter, border, patch), *auto, stats)
        else:
            self._call(be, "msclean", shape[0], psf, image, model, *sc,
                       *clean_scalars(gain, threshold, niter, border, patch), stats)
        del keep
        return model, image, stats

    def mfclean(self, images, psfs, gain=0.1, threshold=0.0, niter=100, border=0, patch=0, models=None):
        """Multi-term CLEAN of the T residual images `images` ([T, N, N] float64, 1 <= T <= 4) with the 2T - 1 spectral
        PSFs `psfs` ([2T - 1, N, N]) (gridhip_mfclean[_dev]; include/gridhip.h, "wide-band imaging"): at most niter
        components, each the T Taylor coefficients at the cell with the largest Hessian-weighted score, searched inside
        `border`, stopping at |a_0| <= threshold; region and patch as for clean.  `images` is UPDATED IN PLACE and
        returned as the residuals; `models` ([T, N, N], zeros when None) is accumulated into.  Returns (models,
        residuals, stats); stats = [iterations, a_0 at the final peak, its flat index, flux_0 .. flux_3, reason] with
        reason 0 niter taken, 1 threshold, 2 nothing selectable, 3 singular Hessian.  numpy arrays take the synchronous
        host form; torch cuda tensors the asynchronous one on torch's stream, with stats a cuda tensor."""
        be = backend(images)
        shape = tuple(getattr(images, "shape", ()))
        if len(shape) != 3 or shape[1] != shape[2] or not 1 <= shape[0] <= 4:
            raise ValueError("images must be T x N x N with T in 1 .. 4")
        T, N = shape[0], shape[1]
        images = in_place(be, images, shape, "images")
        psfs = be.cv(psfs, be.f64)
        if tuple(psfs.shape) != (2 * T - 1, N, N):
            raise ValueError(f"psfs must be {(2 * T - 1, N, N)}: the 2T - 1 spectral PSFs")
        models = in_place(be, models, shape, "models", images)
        stats = be.empty(8, be.f64, images)
        self._call(be, "mfclean", N, T, psfs, images, models, *clean_scalars(gain, threshold, niter, border, patch), stats)
        return models, images, stats

    def jclean(self, images, psfs, metric="sumsq", weights=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0,
               models=None, mask=None, nsigma=0.0, noise=None, peak_frac=0.0):
        """Joint CLEAN of the P images `images` ([P, N, N] float64, 1 <= P <= 8) of one sky - Stokes planes, channels -
        (gridhip_jclean[_dev]; include/gridhip.h, "joint deconvolution"): the search runs on one statistic, metric "sum":
        s = sum_p w_p R_p, or "sumsq": s = sum_p w_p R_p^2, and every component is taken at one cell in all planes, plane
        p losing gain * R_p[k] times its PSF.  `psfs` is [N, N] or [1, N, N] - one PSF for all planes - or [P, N, N], one
        per plane.  `weights`: P host numbers, finite and >= 0 (a plane of weight 0 does not steer the search and is
        still cleaned); None is 1 / P each for "sum" - the mean image, so that thresholds stay in image units - and 1
        each for "sumsq".  The loop stops at |s| <= L = max(threshold^d, (nsigma * sigma)^d, peak_frac^d * |first s|),
        d = 1 for "sum" and 2 for "sumsq": the levels are given in image units.  border, patch, mask, nsigma, noise and
        peak_frac as for clean.  `images` is UPDATED IN PLACE and returned as the residuals; `models` ([P, N, N], zeros
        when None) is accumulated into.  Returns (models, residuals, stats); stats = [iterations, s at the final peak,
        its flat index, L, reason, first s, 0, 0, flux_0 .. flux_7] with clean's reasons.  numpy arrays take the
        synchronous host form; torch cuda tensors the asynchronous one on torch's stream, with stats a cuda tensor.  As
        for clean, a numeric `noise` with cuda tensors is a host-to-device copy and cannot be captured: pass a device
        element such as image_stats(...)[3:4]."""
        be = backend(images)
        shape = tuple(getattr(images, "shape", ()))
        if len(shape) != 3 or shape[1] != shape[2] or not 1 <= shape[0] <= JOINT_MAX_PLANES:
            raise ValueError(f"images must be P x N x N with P in 1 .. {JOINT_MAX_PLANES}")
        P, N = shape[0], shape[1]
        images = in_place(be, images, shape, "images")
        Q, psfs = psf_planes(be, psfs, P, N)
        search, keep = joint_search(metric, weights, P)
        models = in_place(be, models, shape, "models", images)
        auto = auto_args(be, mask, nsigma, noise, peak_frac, (N, N), images) or (None, 0.0, None, 0.0)
        stats = be.empty(16, be.f64, images)
        self._call(be, "jclean", N, P, Q, psfs, images, models, *search,
                   *clean_scalars(gain, threshold, niter, border, patch), *auto, stats)
        del keep
        return models, images, stats

    def fit_beam(self, psf, window=8, cut=0.5):
        """The restoring beam of the N x N `psf` (gridhip_fit_beam[_dev]; include/gridhip.h, "restoring beam and
        restore"): an elliptical Gaussian fitted to the main lobe over the cells within `window` of the centre that
        reach `cut` of the peak (and the centre's eight neighbours).  Returns the 8 values [A, B, C, bmaj, bmin, bpa,
        ncells, ok] - FWHMs in cells (a cell is theta / N radians), bpa in radians from +x towards +y; ok = 0 and NaNs
        when the fit failed.  A numpy psf takes the synchronous host form; a torch cuda tensor the asynchronous one,
        and the result is a cuda tensor: nothing is read back."""
        be = backend(psf)
        psf = be.cv(psf, be.f64)
        shape = tuple(psf.shape)
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("psf must be N x N")
        beam = be.empty(8, be.f64, psf)
        self._call(be, "fit_beam", shape[0], psf, int(window), float(cut), beam)
        return beam

    def restore(self, model, residual, beam, support=None, out=None):
        """restored = model convolved with the beam + residual (gridhip_restore[_dev]), in units per beam: `model` and
        `residual` are N x N float64 as clean returns them, `beam` the 8 values of fit_beam (or [A, B, C, 0, 0, 0, 0, 1]
        of your own), `support` the half-width of the convolution in cells, 1 to 32.  support=None derives it from the
        beam - the smallest R with exp(-lambda_min R^2) <= 1e-9 - which READS THE BEAM BACK: one synchronisation for
        cuda tensors, and a ValueError when the fit failed or R exceeds 32; an explicit support keeps the call
        asynchronous (a failed beam then gives an all-NaN image from the device form).  out: the array to write (a new
        one when None); it may be `residual` itself.  Returns it."""
        be = backend(model)
        shape = tuple(getattr(model, "shape", ()))
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("model must be N x N")
        model, residual = image_of(be, model, shape, "model"), image_of(be, residual, shape, "residual")
        beam = be.cv(beam, be.f64)
        if tuple(beam.shape) != (8,):
            raise ValueError("beam must be the 8 values of fit_beam")
        out = be.empty(shape, be.f64, model) if out is None else in_place(be, out, shape, "out")
        if support is None:
            support = beam_support(beam.tolist())
        self._call(be, "restore", shape[0], model, residual, beam, int(support), out)
        return out

    def weights(self, theta, lam, p, mode="uniform", robust=0.0, taper=0.0, weights=None, out=None):
        """Imaging weights of the baselines `p` (wavelengths, taken as given: mirror first for Hermitian cells; a (u, v[, w])
        tuple or an (n, 3) array) on the N x N grid of image_size(theta, lam) (gridhip_weights[_dev]; include/gridhip.h,
        "imaging weights"): mode "natural" | "uniform" | "briggs" with `robust`, a Gaussian taper of sigma `taper`
        wavelengths (0: none) and the data weights `weights` (None: ones; a value that is not > 0 flags its visibility,
        whose weight is exactly 0).  Returns (w, stats): n float64 weights and the 8 values [sum w, sum w^2 / s, sum s,
        noise, f^2, n_used, n_flagged, n_outside].  out: the array to write (a new one when None); it may be `weights`
        itself.  numpy arrays take the synchronous host form; torch cuda tensors the asynchronous one on torch's stream,
        and both results are cuda tensors: nothing is read back."""
        be = backend(p[0] if isinstance(p, (tuple, list)) else p)
        u, v, st = baselines(be, p, 2)
        n = int(u.shape[0])
        m, robust, taper, wt = _weighting(be, mode, robust, taper, weights, n)
        if out is None:
            out = be.empty(n, be.f64, u)
        elif not (be is backend(out) and be.ok(out, be.f64) and tuple(out.shape) == (n,)):
            raise ValueError(f"out must be {be.form.replace('complex128', 'float64')} of shape ({n},)")
        stats = be.empty(8, be.f64, u)
        self._call(be, "weights", float(theta), int(lam), n, u, v, st, wt, m, robust, taper, out, stats)
        return out, stats

    def gaincal(self, vis, model_vis, a1, a2, nant, *, slot=None, nslots=1, weights=None, phase_only=False, refant=0,
                niter=50, tol=1e-8, gains=None):
        """Antenna gains of `vis` against `model_vis` by StEFCal (gridhip_gaincal[_dev]; include/gridhip.h, "gain
        calibration"): vis ~ g[slot, a1] model_vis conj(g[slot, a2]) for n visibilities, `nant` antennas and `nslots`
        solution intervals (slot None: one interval).  weights: n data weights (None: ones; a value that is not > 0 flags
        its visibility, which then contributes nothing even where it is NaN).  phase_only keeps |g| = 1; refant: the
        antenna whose gain is made real and non-negative in every interval (None: no rotation); at most niter iterations,
        stopped on the device once the relative change is <= tol (tol = 0: never early).  gains: an (nslots, nant)
        complex128 array in the ABI's form to start from (a warm start) - it is updated in place and returned - or None to
        start from 1.  Returns (gains, stats), stats the 8 values [iterations, last rel, chi^2, chi^2 at g = 1, n_used,
        n_flagged, n_dropped, n_unsolved].  numpy arrays take the synchronous host form; torch cuda tensors the
        asynchronous one on torch's stream, and both results are cuda tensors: nothing is read back."""
        be = backend(vis)
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, nant, slot, nslots, weights)
        model_vis = stream_array(be, model_vis, be.c128, n, "model_vis")
        mode, refant, warm, niter, tol, gains = solve_args(be, phase_only, refant, niter, tol, gains, A, T, vis)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "gaincal", n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
        return gains, stats

    def ddcal(self, vis, model_vis, a1, a2, nant, *, slot=None, nslots=1, weights=None, phase_only=False, refant=0,
              niter=50, tol=1e-8, gains=None):
        """Direction-dependent gains of `vis` against the D rows of `model_vis` (D, n) by the multi-direction StEFCal
        (gridhip_ddcal[_dev]; include/gridhip.h, "direction-dependent calibration"): vis ~ sum over d of g[d, slot, a1]
        model_vis[d] conj(g[d, slot, a2]).  Everything else is Context.gaincal's; an (slot, antenna) whose D x D normal
        matrix has a pivot at or below 1e-12 of its diagonal keeps all its gains.  gains: a (D, nslots, nant) complex128
        array in the ABI's form to start from, updated in place, or None.  Returns (gains (D, nslots, nant), stats)."""
        be = backend(vis)
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, nant, slot, nslots, weights)
        D, model_vis = model_rows(be, model_vis, n)
        mode, refant, warm, niter, tol, gains = solve_args(be, phase_only, refant, niter, tol, gains, A, T, vis, D)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "ddcal", n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
        return gains, stats

    def dd_subtract(self, gains, model_vis, a1, a2, *, slot=None, directions=None, vis=None, out=None):
        """vis minus the corrupted models of `directions` (an iterable of direction numbers; None: all):
        vis - sum over d of g[d, slot, a1] model_vis[d] conj(g[d, slot, a2]) with the (D, nslots, nant) gains
        (gridhip_dd_subtract[_dev]).  vis None: plus that sum - the corrupted model itself.  A visibility whose indices
        are out of range keeps its value.  out: the array to write (a new one when None); it may be `vis`.  Correcting
        toward direction d afterwards is Context.apply_gains(gains[d], ...)."""
        be = backend(model_vis)
        if not hasattr(gains, "shape") or len(gains.shape) != 3:
            raise ValueError("gains must be of shape (D, nslots, nant)")
        D, T, A = (int(v) for v in gains.shape)
        Dm, model_vis = model_rows(be, model_vis, -1)
        if Dm != D:
            raise ValueError(f"gains has {D} directions and model_vis {Dm}")
        n, A, T, a1, a2, slot, first, _ = gain_stream(be, model_vis[0] if vis is None else vis, a1, a2, A, slot, T, None)
        if int(model_vis.shape[1]) != n:
            raise ValueError("model_vis must have one column per visibility")
        gains = stream_array(be, gains.reshape(-1), be.c128, D * T * A, "gains")
        out = result_array(be, out, be.c128, (n,), "out", model_vis)
        self._call(be, "dd_subtract", n, A, T, D, a1, a2, slot, gains, model_vis, direction_mask(directions, D),
                   None if vis is None else first, out)
        return out

    def apply_gains(self, gains, vis, a1, a2, *, slot=None, inverse=True, weights=None, out=None, weights_out=None):
        """Apply the (nslots, nant) gains to a visibility stream (gridhip_apply_gains[_dev]).  inverse=True corrects data:
        vis / (g[slot, a1] conj(g[slot, a2])) and weights |g[a1]|^2 |g[a2]|^2 times `weights` (None: ones); a visibility
        whose indices are out of range or whose gains are zero or not finite keeps its value and gets the weight +0.0,
        the flag of Context.weights.  inverse=False corrupts a model: g[a1] vis conj(g[a2]), weights copied.  out and
        weights_out: the arrays to write (new ones when None); they may be `vis` and `weights` themselves.  Returns
        (vis_out, weights_out)."""
        be = backend(vis)
        if not hasattr(gains, "shape") or len(gains.shape) != 2:
            raise ValueError("gains must be of shape (nslots, nant)")
        T, A = int(gains.shape[0]), int(gains.shape[1])
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, A, slot, T, weights)
        gains = stream_array(be, gains.reshape(-1), be.c128, T * A, "gains")
        out = result_array(be, out, be.c128, (n,), "out", vis)
        weights_out = result_array(be, weights_out, be.f64, (n,), "weights_out", vis)
        self._call(be, "apply_gains", n, A, T, a1, a2, slot, gains, int(bool(inverse)), vis, wt, out, weights_out)
        return out, weights_out

    def jonescal(self, vis, model_vis, a1, a2, nant, *, slot=None, nslots=1, weights=None, mode="full", refant=0, niter=50,
                 tol=1e-8, gains=None):
        """Jones matrices of the four-correlation stream `vis` (n, 2, 2) against `model_vis` (n, 2, 2) by the matrix
        StEFCal (gridhip_jonescal[_dev]; include/gridhip.h, "polarisation"): vis ~ G[slot, a1] model_vis G[slot, a2]^H.
        mode: "full" (a 2x2 matrix per antenna), "diagonal" (one gain per feed, solved over all four correlations) or
        "phase" (diagonal, |g| = 1).  weights: one per sample, shared by its four correlations.  refant: the antenna
        whose [0][0] entry is made real and non-negative in every interval - only a common phase is taken out (None:
        nothing).  gains: an (nslots, nant, 2, 2) complex128 array in the ABI's form to start from, updated in place, or
        None to start from the identity.  Everything else is Context.gaincal's.  Returns (gains (nslots, nant, 2, 2),
        stats), stats the 8 values of Context.gaincal."""
        be = backend(vis)
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, nant, slot, nslots, weights, jones=True)
        model_vis = jones_array(be, model_vis, n, "model_vis")
        mode, refant, warm, niter, tol, gains = solve_args(be, mode, refant, niter, tol, gains, A, T, vis, "jones")
        stats = be.empty(8, be.f64, vis)
        self._call(be, "jonescal", n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
        return gains, stats

    def apply_jones(self, gains, vis, a1, a2, *, slot=None, weights=None, inverse=True, out=None, weights_out=None):
        """Apply the (nslots, nant, 2, 2) Jones matrices to a four-correlation stream (n, 2, 2)
        (gridhip_apply_jones[_dev]).  inverse=True corrects data: G[a1]^-1 vis G[a2]^-H and weights |det G[a1]|
        |det G[a2]| times `weights` (None: ones); a sample whose indices are out of range or that touches a matrix whose
        |det|^2 is zero or not finite keeps its value and gets the weight +0.0.  inverse=False corrupts a model:
        G[a1] vis G[a2]^H, weights copied.  out and weights_out: the arrays to write (new ones when None); they may be
        `vis` and `weights` themselves.  Returns (vis_out, weights_out)."""
        be = backend(vis)
        if not hasattr(gains, "shape") or len(gains.shape) != 4 or tuple(gains.shape[2:]) != (2, 2):
            raise ValueError("gains must be of shape (nslots, nant, 2, 2)")
        T, A = int(gains.shape[0]), int(gains.shape[1])
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, A, slot, T, weights, jones=True)
        gains = jones_array(be, gains.reshape(T * A, 2, 2), T * A, "gains")
        out = result_array(be, out, be.c128, (n, 2, 2), "out", vis)
        weights_out = result_array(be, weights_out, be.f64, (n,), "weights_out", vis)
        self._call(be, "apply_jones", n, A, T, a1, a2, slot, gains, int(bool(inverse)), vis, wt, out, weights_out)
        return out, weights_out

    def stokes(self, vis, basis="linear", which="IQUV", inverse=False, out=None):
        """Correlations <-> Stokes parameters (gridhip_stokes[_dev]).  Forward: `vis` (n, 2, 2) -> the (4, n) block of
        the rows I, Q, U, V, of which those named in `which` are written - each row is a contiguous stream for
        Context.imager, weights, flag_residuals, average or gaincal; out: the block to write into (its other rows are
        not touched), or None for a new one of zeros.  inverse=True: `vis` is the (4, n) block, all four rows, and the
        result the (n, 2, 2) stream - how four per-Stokes predictions become the model_vis of Context.jonescal.
        basis: "linear" (XX, XY, YX, YY) or "circular" (RR, RL, LR, LL).  The one weight per sample serves all four
        streams."""
        be = backend(vis)
        args, out = stokes_args(be, vis, basis, which, inverse, out)
        self._call(be, "stokes", *args)
        return out

    def flag_residuals(self, vis, model_vis=None, group=None, G=None, weights=None, nsigma=5.0, amax=0.0, min_count=8,
                       niter=3, out=None):
        """Robust per-group flagging of the residuals vis - model_vis (gridhip_flag_residuals[_dev]; include/gridhip.h,
        "residual flagging"): per group the lower median and the MAD of the amplitudes a = sqrt(re^2 + im^2), and in each
        of at most niter rounds a sample with a > med + nsigma * 1.4826 * MAD is clipped (a group of fewer than min_count
        samples or with MAD = 0 is not).  model_vis None: zero.  group: the group of every visibility in [0, G) (a sample
        whose group is outside is left alone), as flag_groups returns it with G; None: one group.  weights: n data
        weights (None: ones; a value that is not > 0 flags its visibility on input).  amax > 0 also flags a > amax.
        Returns (weights, flags, group_stats, stats): the weights with +0.0 where a sample was flagged (out: the array to
        write, which may be `weights` itself), the class of every sample (uint8: 0 kept, 1 flagged on input, 2 left alone,
        3 not finite, 4 above amax, 16 + r clipped in round r), the (G, 4) values [n, median, MAD, T] per group of the last
        round that ran, and the 8 values [rounds, participants, clipped, not finite, above amax, left alone, flagged on
        input, kept].  The result is an order statistic throughout: the same bits on every run.  numpy arrays take the
        synchronous host form; torch cuda tensors the asynchronous one on torch's stream, and every result is a cuda
        tensor: nothing is read back."""
        be = backend(vis)
        n, G, group, vis, model_vis, wt = flag_stream(be, vis, model_vis, group, G, weights)
        scalars = flag_scalars(nsigma, amax, min_count, niter)
        out, flags, gstats, stats = flag_outputs(be, n, G, out, vis)
        self._call(be, "flag_residuals", n, G, group, vis, model_vis, wt, *scalars, out, flags, gstats, stats)
        return out, flags, gstats, stats

    def sumthreshold(self, vis, model_vis=None, weights=None, order="btf", levels=None, nsigma=6.0, rho=1.5, nlevels=7,
                     eta=(0.2, 0.2), min_count=8, niter=2, out=None):
        """Time-frequency flagging of a cube of residuals vis - model_vis (gridhip_sumthreshold[_dev]; include/gridhip.h,
        "time-frequency flagging"): SumThreshold with the windows 1, 2, 4, ... along frequency and time against
        levels[k] * sigma_b, sigma_b from the lower median and the MAD of every baseline, in up to niter rounds, then the
        SIR operator along frequency with eta[0] and along time with eta[1] (0: skipped).  vis is three-dimensional:
        [B][T][F] for order "btf", [T][B][F] for "tbf"; model_vis and weights have its shape (None: zero; ones - a weight
        that is not > 0 flags its sample on input, and a cell that holds no measurement carries 0).  levels None: the
        ladder nsigma / rho^k, k < nlevels.  Returns (weights, flags, baseline_stats, stats): the weights with +0.0 where
        a sample is flagged (out: the array to write, which may be `weights` itself) and the code of every sample (uint8:
        0 kept, 1 flagged on input, 3 not finite, 8 added by SIR, 16 + 8 r + k by stage k of round r), both shaped as vis;
        (B, 4) rows [n, median, MAD, chi_0] of the last round that ran; and the 8 values [rounds, participants, flagged by
        SumThreshold, not finite, added by SIR, 0, flagged on input, kept].  numpy arrays take the synchronous host form;
        torch cuda tensors the asynchronous device form on torch's current stream, which reads nothing back."""
        be = backend(vis)
        cube, shape = cube_arrays(be, vis, model_vis, weights, order)
        K, levels, *scalars = sumthreshold_scalars(levels, nsigma, rho, nlevels, eta, min_count, niter)
        n, B = shape[0] * shape[1] * shape[2], cube[0]
        given = out  # (written in place and returned as it is)
        out, flags, bstats, stats = flag_outputs(be, n, B, None if out is None else result_array(
            be, out, be.f64, shape, "out", vis).reshape(n), cube[4])
        self._call(be, "sumthreshold", *cube, K, levels.ctypes.data_as(C.POINTER(C.c_double)), *scalars, out, flags, bstats,
                   stats)
        return out.reshape(shape) if given is None else given, flags.reshape(shape), bstats, stats

    def rm_tables(self, lam2, phi, weights=None, fwhm=None):
        """The table RM synthesis and RM-CLEAN read (gridhip_rm_tables[_dev]; include/gridhip.h, "rotation-measure
        synthesis"): lam2 - the C <= 1024 squared wavelengths of the channels - weights (C values, finite and >= 0; None:
        ones) and the Faraday depths phi = (phi0, dphi, J), phi_j = phi0 + j dphi, J <= 512 (gridhip.faraday_grid proposes
        them).  fwhm: the width of the restoring Gaussian; None: 2 sqrt(3) / (max lam2 - min lam2).  Returns one float64
        array of 16 + 2 C J + 3 (2 J - 1) values: the head [valid, C, J, phi0, dphi, lam0^2, K, sum w, fwhm, 0 ...], the
        phasors E[C][J] with the weights folded in, the RMSF R[2J - 1] and the restoring function G[2J - 1].  lam2 and the
        weights are judged on the device: a value that is not finite, a negative weight or no weight above 0 gives
        valid = 0, which rmsynth and rmclean report in stats[7].  A numpy lam2 takes the synchronous host form; a torch
        cuda tensor the asynchronous one on torch's stream (fwhm=None reads lam2's range back, once)."""
        be = backend(lam2)
        C_, J, lam2, weights, phi0, dphi, fwhm = rm_table_args(be, lam2, phi, weights, fwhm)
        tables = be.empty(rm_table_doubles(C_, J), be.f64, lam2)
        self._call(be, "rm_tables", C_, J, lam2, weights, phi0, dphi, fwhm, tables)
        return tables

    def rmsynth(self, q, u, tables, out=None):
        """RM synthesis (gridhip_rmsynth[_dev]): q and u, real [C, ...] arrays of one shape - the Q and U images of the C
        channels, [C, N, N], or any block of lines of sight such as a slab of rows - give the Faraday dispersion function
        F(phi_j) = sum_c E[c][j] (q_c + i u_c) of every line of sight as a complex128 cube [J, ...], J the table's.
        Returns (cube, stats): stats = [bad, 0, 0, 0, 0, 0, 0, invalid] - a line of sight with a non-finite q or u in any
        channel is NaN at every depth and counted in `bad`; invalid = 1: the table is not valid or not of q's C, and the
        cube was not written.  out: the cube to write.  The same bits on every run and as numpy's unfused products summed
        over the channels in order.  numpy in gives numpy out; torch cuda tensors take the device form on torch's stream."""
        be = backend(q)
        M, C_, q, u, rest = rm_images(be, q, u)
        tables, C_, J = rm_table_of(be, tables, C_=C_)
        cube = result_array(be, out, be.c128, (J,) + rest, "out", q)
        stats = be.empty(8, be.f64, q)
        self._call(be, "rmsynth", M, C_, J, tables, q, u, cube, stats)
        return cube, stats

    def rmclean(self, cube, tables, gain=0.1, threshold=0.0, niter=100, nsigma=0.0, noise=None, restore=False, model=None):
        """RM-CLEAN of every line of sight of `cube` ([J, ...] complex128 as rmsynth returns it; gridhip_rmclean[_dev]): a
        Hogbom loop along the Faraday depth with the table's RMSF - take the depth of the largest |F|^2 (ties to the lowest
        depth), stop when |F| <= L = max(threshold, nsigma * noise) or after niter components, else add gain * F there to
        the model and subtract it times the shifted RMSF.  noise: sigma as a number or one float64 element (a number with
        cuda tensors is uploaded by this call and cannot be captured).  `cube` is UPDATED IN PLACE and returned: the
        residual, or with restore=True the residual plus the whole model convolved with the table's Gaussian.  `model`
        ([J, ...] complex128, zeros when None) is accumulated into.  Returns (model, cube, maps, stats): maps [7, ...] =
        [iterations, reason (0 niter, 1 level, 3 non-finite: left untouched), j*, |F|^2 there, phi fitted by a parabola
        through the three powers around j*, Re F, Im F at j*] of the cube as it is returned; stats = [bad, iterations,
        stopped by niter, stopped at the level, 0, L, NaN noise, invalid table] - either of the last two set: nothing else
        was touched.  Every line of sight is cleaned by one wave, on its own; the same bits on every run."""
        be = backend(cube)
        M, J, rest = rm_cube(be, cube)
        tables, _, J = rm_table_of(be, tables, J=J)
        scalars = rm_clean_scalars(be, gain, threshold, niter, nsigma, noise, restore, cube)
        if model is None:
            model = be.zeros((J,) + rest, be.c128, cube)
        elif not (be is backend(model) and be.ok(model, be.c128) and tuple(model.shape) == tuple(cube.shape)):
            raise ValueError(f"model must be {be.form} of the cube's shape (it is accumulated into)")
        maps, stats = be.empty((RM_MAPS,) + rest, be.f64, cube), be.empty(8, be.f64, cube)
        self._call(be, "rmclean", M, J, tables, cube, model, *scalars, maps, stats)
        return model, cube, maps, stats

    def contsub(self, data, x, mask=None, weights=None, degree=1, axis=-1, mode="subtract", nsigma=0.0, niter=0, out=None,
                coeffs=True, info=True, codes=False):
        """Continuum subtraction (gridhip_contsub[_dev]; include/gridhip.h, "continuum subtraction"): per spectrum a
        Chebyshev polynomial of `degree` <= 3 in the channel coordinate x (C values; gridhip.channel_coordinate), fitted by
        weighted least squares to the samples that `mask` (C values, non-zero: a line-free channel; None: all) and
        `weights` (data's shape; a weight that is not finite and > 0 drops its sample: the per-row mask) let in, with up to
        niter <= 4 rounds that drop the samples whose weighted squared residual exceeds nsigma^2 times the row's mean and
        fit again.  data: [..., C] for axis=-1 - a sumthreshold cube in either order - or [C, ...] for axis=0 - an image
        cube; complex128 or float64, in the ABI's form: nothing is converted, transposed or copied.  mode "subtract": out =
        data - continuum; "model": out = the continuum, at every channel of every spectrum.  out: the array to write,
        which may be data itself; a new one when None.  Returns (out, coeffs, info, codes, stats): coeffs [..., D+1] or
        [D+1, ...] of data's dtype (for axis=0 coefficient images; a row that fell back has +0.0 above its degree); info
        [..., 4] or [4, ...] = [degree used (-1: no usable sample, continuum 0), samples in the final fit, samples clipped,
        final mean weighted squared residual]; codes (uint8, data's shape: 0 used, 1 flagged on input, 3 not finite, 2
        masked, 16 + i clipped in round i); stats = [rows, at full degree, at reduced degree, without a fit, samples used,
        clipped, not finite, flagged on input].  coeffs, info, codes False: that output is not made (None comes back).  A
        channel whose x is not finite is NaN in out.  The same bits on every run, for both axes of the same cube and as
        tests/contsub_ref.py.  numpy in gives numpy out; torch cuda tensors take the device form on torch's stream: three
        launches, nothing read back."""
        be = backend(data)
        args = contsub_args(be, data, x, mask, weights, degree, axis, mode, nsigma, niter, out, coeffs, info, codes)
        self._call(be, "contsub", *args)
        return args[12:]

    def fringe_tables(self, freq, time, tint, delays, rates):
        """The table the fringe search and the apply step read (gridhip_fringe_tables[_dev]; include/gridhip.h, "delay and
        rate calibration"): freq (F <= 1024 channels, Hz) and time (T steps, seconds), neither necessarily uniform; tint
        time steps per solution interval (0: all T; at most 256); delays = (tau0, dtau, Nd <= 4096) and rates = (r0, drate,
        Nr <= 1024), the cells tau_j = tau0 + j dtau and r_k = r0 + k drate (gridhip.fringe_grid proposes them).  Returns one
        float64 array: the head [valid, F, T, tint, I, Nd, Nr, tau0, dtau, r0, drate, nu0, 0 ...], the phasors Ef[F][Nd] and
        Et[T][Nr], the reference times, nu_f - nu0 and t - tref.  freq and time are judged on the device: a value that is
        not finite, or a step that is not > 0, gives valid = 0, which every reader reports.  numpy in gives numpy out; torch
        cuda tensors take the device form on torch's stream."""
        be = backend(freq)
        args = fringe_table_args(be, freq, time, tint, delays, rates)
        tables = be.empty(fringe_table_doubles(args[0], args[1], args[7], args[10]), be.f64, args[3])
        self._call(be, "fringe_tables", *args, tables)
        return tables

    def fringe_search(self, vis, tables, a1, a2, nant, tint, delays, rates, model_vis=None, weights=None, sol=None, cells=None,
                      peaks=None):
        """The fringe search (gridhip_fringe_search[_dev]): per baseline of the [B, T, F] cube `vis` and solution interval,
        the delay and rate cell at which sum_t Et[t][k] sum_f Ef[f][j] X'[t][f] has the largest power, X' = weights * vis *
        conj(model_vis), derotated by `sol` ([I, nant, 4] = tau, r, Re g, Im g) where one is given.  a1, a2: the B antenna
        pairs; tint, delays = (tau0, dtau, Nd) and rates = (r0, drate, Nr): what the table was made with; cells = (j0, j1, k0,
        k1): the half-open ranges of delay and rate cells to search (None: the whole grid).  Returns (peaks [B, I, 12], stats): a row is [j*, k*,
        P*, tau_b, r_b, Re z, Im z, coh2, n_used, N, code, 0] with the peak refined by a parabola per axis where it is
        interior to the ranges, z the unit phasor of the peak, coh2 = P* / (n_used N) in [0, 1] and code 0 ok, 1 no
        unflagged sample, 2 a non-finite unflagged sample, 3 p == q or an antenna out of range; stats = [flagged samples,
        bad, empty, refused, ok rows, 0, 0, invalid] - invalid = 1: the table does not belong to this cube, was made with another
        tint, or the cells do not lie in its grid, and peaks was not written.  A sample whose weight is not > 0 contributes exactly nothing.  The same
        bits on every run and as tests/fringe_ref.py given the table."""
        be = backend(vis)
        B, T, F, A, vis, model_vis, wt, a1, a2 = fringe_cube(be, vis, model_vis, weights, a1, a2, nant)
        tables, I = fringe_table_of(be, tables, F, T, tint)
        Nd, Nr = int(delays[2]), int(rates[2])
        if int(tables.shape[0]) != fringe_table_doubles(F, T, Nd, Nr):
            raise ValueError(f"tables of {int(tables.shape[0])} values do not belong to this cube and these axes")
        try:
            j0, j1, k0, k1 = (0, Nd, 0, Nr) if cells is None else (int(v) for v in cells)
        except (TypeError, ValueError):
            raise ValueError("cells must be (j0, j1, k0, k1)") from None
        if not (0 <= j0 < j1 <= Nd and 0 <= k0 < k1 <= Nr):
            raise ValueError("cells must be half-open ranges 0 <= j0 < j1 and 0 <= k0 < k1 inside the grid")
        sol = fringe_sol(be, sol, I, A, vis)
        peaks = result_array(be, peaks, be.f64, (B, I, FRINGE_PEAK), "peaks", vis)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "fringe_search", B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats)
        return peaks, stats

    def fringe_solve(self, peaks, a1, a2, nant, sol=None, min_count=0, min_coh2=0.0, refant=0, niter=50, tol=0.0):
        """The antenna-based fit of the baseline values of a fringe search (gridhip_fringe_solve[_dev]): per interval,
        Jacobi sweeps on the weighted least squares of tau_p - tau_q = tau_b and r_p - r_q = r_b and a phase-only StEFCal
        on the peak phasors, all weighted by coh2 of the baselines with code 0, n_used >= min_count and coh2 >= min_coh2;
        then referenced to `refant` (None: not) and ACCUMULATED into `sol` ([I, nant, 4]; None: a new one of tau = r = 0,
        g = 1), which is returned: (sol, info [I, nant] - the used baselines per antenna, 0: unsolved and untouched -
        stats = [sweeps, used baselines, unsolved antennas, unreferenced intervals, rms tau_b, rms r_b, 0, 0]).  The sweeps
        stop when the largest change of each of the three is at or below tol (relative to the largest value for delays
        and rates).  No floating-point atomic: the same bits on every run and as tests/fringe_ref.py."""
        be = backend(peaks)
        shape = tuple(int(v) for v in getattr(peaks, "shape", ()))
        if not (hasattr(peaks, "dtype") and be.ok(peaks, be.f64)) or len(shape) != 3 or shape[2] != FRINGE_PEAK or min(shape) < 1:
            raise ValueError(f"peaks must be a float64 {be.array} of shape [B, I, {FRINGE_PEAK}] (Context.fringe_search)")
        B, I, A = shape[0], shape[1], int(nant)
        if A < 2:
            raise ValueError("nant must be >= 2")
        a1, a2 = stream_array(be, a1, be.i64, B, "a1"), stream_array(be, a2, be.i64, B, "a2")
        scalars = fringe_solve_scalars(min_count, min_coh2, refant, niter, tol, A)
        if sol is None:
            sol = be.zeros((I, A, 4), be.f64, peaks)
            sol[:, :, 2] = 1.0
        sol = fringe_sol(be, sol, I, A, peaks)
        info, stats = be.empty((I, A), be.f64, peaks), be.empty(8, be.f64, peaks)
        self._call(be, "fringe_solve", B, I, A, a1, a2, peaks, *scalars, sol, info, stats)
        return sol, info, stats

    def fringefit(self, vis, tables, a1, a2, nant, tint, delays, rates, model_vis=None, weights=None, sol=None, rounds=3,
                  window=(2, 2), min_count=0, min_coh2=0.0, refant=0, niter=50, tol=0.0):
        """Delay and rate calibration (gridhip_fringefit[_dev]): `rounds` (1 .. 4) times a fringe search followed by the
        antenna-based fit.  Round 0 searches the whole grid - delays = (tau0, dtau, Nd), rates = (r0, drate, Nr) and tint
        as given to Context.fringe_tables - against `sol` where one is given (a warm start, updated in place) or zero; the
        later rounds derotate by the current solution and search only the cells within window = (wj, wk) of the grid's
        zero, so that the parabola refines a residual of a fraction of a cell.  Everything else is Context.fringe_search's
        and Context.fringe_solve's.  Returns (sol [I, nant, 4] = tau, r, Re g, Im g per interval and antenna, peaks of the
        last round, info, stats = [sweeps of the last solve, flagged samples, bad, empty, unsolved antennas, weighted rms
        of the last round's tau_b and r_b in cells, invalid]).  Correct data with Context.apply_fringe(sol, ...).  A fixed
        number of launches, nothing read back: with cuda tensors the call can be captured into a graph."""
        be = backend(vis)
        B, T, F, A, vis, model_vis, wt, a1, a2 = fringe_cube(be, vis, model_vis, weights, a1, a2, nant)
        tables, I = fringe_table_of(be, tables, F, T, tint)
        Nd, Nr = int(delays[2]), int(rates[2])
        if int(tables.shape[0]) != fringe_table_doubles(F, T, Nd, Nr):
            raise ValueError(f"tables of {int(tables.shape[0])} values do not belong to this cube and these axes")
        rounds, (wj, wk) = int(rounds), (int(v) for v in window)
        if not 1 <= rounds <= 4 or not (0 <= wj <= FRINGE_MAX_DELAYS and 0 <= wk <= FRINGE_MAX_RATES):
            raise ValueError("rounds must be in 1 .. 4 and window a pair of cell counts >= 0")
        scalars = fringe_solve_scalars(min_count, min_coh2, refant, niter, tol, A)
        warm = int(sol is not None)
        sol = fringe_sol(be, sol, I, A, vis) if warm else be.empty((I, A, 4), be.f64, vis)
        peaks, info = be.empty((B, I, FRINGE_PEAK), be.f64, vis), be.empty((I, A), be.f64, vis)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "fringefit", B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, *scalars,
                   warm, sol, peaks, info, stats)
        return sol, peaks, info, stats

    def apply_fringe(self, sol, tables, vis, a1, a2, tint, *, inverse=True, weights=None, out=None, weights_out=None):
        """Apply a delay and rate solution to a [B, T, F] cube (gridhip_apply_fringe[_dev]).  inverse=True corrects data:
        vis conj(D) with D = g_p conj(g_q) exp(2 pi i ((tau_p - tau_q)(nu_f - nu0) + (r_p - r_q)(t - tref_i))); inverse=False
        corrupts a model: vis D.  Weights are copied (ones without `weights`); a sample that touches an antenna whose row
        of `sol` is not finite, or an antenna out of range, keeps its value and gets the weight +0.0.  out, weights_out:
        the arrays to write, which may be vis and weights themselves.  Returns (out, weights_out); a table made with another tint
        than the one given here leaves both unwritten (a numpy table is refused with ValueError).  Only the head and the
        two coordinate vectors of the table are read: a table of any search axes over the same freq, time and tint."""
        be = backend(vis)
        nant = int(sol.shape[1]) if hasattr(sol, "shape") and len(sol.shape) == 3 else 0
        B, T, F, A, vis, _, wt, a1, a2 = fringe_cube(be, vis, None, weights, a1, a2, nant)
        tables, I = fringe_table_of(be, tables, F, T, tint)
        sol = fringe_sol(be, sol, I, A, vis)
        out = result_array(be, out, be.c128, (B, T, F), "out", vis)
        weights_out = result_array(be, weights_out, be.f64, (B, T, F), "weights_out", vis)
        self._call(be, "apply_fringe", B, T, F, A, I, tables, sol, a1, a2, int(bool(inverse)), vis, wt, out, weights_out)
        return out, weights_out

    def tec_tables(self, freq, ntime, tint, delays, tecs):
        """The table the delay-TEC search and its apply step read (gridhip_tec_tables[_dev]; include/gridhip.h, "dispersive
        delay (TEC) calibration"): freq (F <= 1024 channels, Hz, every one > 0), ntime = T time steps of the cube and tint
        of them per solution interval (0: all; no other cap), delays = (tau0, dtau, Nd <= 4096) and tecs = (tec0, dtec,
        Nm <= 1024) in TEC units (gridhip.tec_grid proposes both).  Returns one float64 array: the head [valid, F, T, tint, I,
        Nd, Nm, tau0, dtau, tec0, dtec, nu0, s, kappa, 0, 0], the phasors Ef[F][Nd] and Em[F][Nm], a_f = nu_f - nu0 and the
        orthogonalised dispersive coordinate c_f = z_f - s a_f.  freq is judged on the device: valid = 0 is what every
        reader reports.  numpy in gives numpy out; torch cuda tensors take the device form on torch's stream."""
        be = backend(freq)
        args = tec_table_args(be, freq, ntime, tint, delays, tecs)
        tables = be.empty(tec_table_doubles(args[0], args[6], args[9]), be.f64, args[3])
        self._call(be, "tec_tables", *args, tables)
        return tables

    def tec_search(self, vis, tables, a1, a2, nant, tint, delays, tecs, model_vis=None, weights=None, sol=None, cells=None,
                   peaks=None):
        """The delay-TEC search (gridhip_tec_search[_dev]): per baseline of the [B, T, F] cube `vis` and solution interval,
        the delay and TEC cell at which sum_f Ef[f][j] Em[f][m] Xbar[f] has the largest power, Xbar the sum over the
        interval of X' = weights * vis * conj(model_vis), derotated by `sol` ([I, nant, 4] = tau, tec, Re g, Im g) where
        one is given.  Arguments, cells = (j0, j1, m0, m1), the returned (peaks [B, I, 12], stats), the codes and the
        refusals are Context.fringe_search's, with the TEC axis for the rate axis: a row is [j*, m*, P*, tau_b, tec_b,
        Re z, Im z, coh2, n_used, N, code, 0].  The delay is the effective one, tau_clock + s tec (gridhip.tec_clock).  The
        same bits on every run and as tests/tec_ref.py given the table."""
        be = backend(vis)
        B, T, F, A, vis, model_vis, wt, a1, a2 = fringe_cube(be, vis, model_vis, weights, a1, a2, nant)
        tables, I = tec_table_of(be, tables, F, T, tint)
        Nd, Nm = int(delays[2]), int(tecs[2])
        if int(tables.shape[0]) != tec_table_doubles(F, Nd, Nm):
            raise ValueError(f"tables of {int(tables.shape[0])} values do not belong to this cube and these axes")
        try:
            j0, j1, m0, m1 = (0, Nd, 0, Nm) if cells is None else (int(v) for v in cells)
        except (TypeError, ValueError):
            raise ValueError("cells must be (j0, j1, m0, m1)") from None
        if not (0 <= j0 < j1 <= Nd and 0 <= m0 < m1 <= Nm):
            raise ValueError("cells must be half-open ranges 0 <= j0 < j1 and 0 <= m0 < m1 inside the grid")
        sol = fringe_sol(be, sol, I, A, vis)
        peaks = result_array(be, peaks, be.f64, (B, I, TEC_PEAK), "peaks", vis)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "tec_search", B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, m0, m1, peaks, stats)
        return peaks, stats

    def tecfit(self, vis, tables, a1, a2, nant, tint, delays, tecs, model_vis=None, weights=None, sol=None, rounds=3,
               window=(2, 2), min_count=0, min_coh2=0.0, refant=0, niter=50, tol=0.0):
        """Dispersive delay calibration (gridhip_tecfit[_dev]): `rounds` (1 .. 4) times a delay-TEC search followed by the
        antenna-based fit of Context.fringe_solve, which serves as it is.  Round 0 searches the whole grid - delays, tecs
        and tint as given to Context.tec_tables - against `sol` where one is given (a warm start, updated in place) or
        zero; the later rounds derotate by the current solution and search only the cells within window = (wj, wm) of the
        grid's zero.  Returns (sol [I, nant, 4] = tau_eff, tec, Re g, Im g per interval and antenna, peaks of the last
        round, info, stats = [sweeps of the last solve, flagged samples, bad, empty, unsolved antennas, weighted rms of the
        last round's tau_b and tec_b in cells, invalid]).  Correct data with Context.apply_tec(sol, ...).  A fixed number
        of launches, nothing read back: with cuda tensors the call can be captured into a graph."""
        be = backend(vis)
        B, T, F, A, vis, model_vis, wt, a1, a2 = fringe_cube(be, vis, model_vis, weights, a1, a2, nant)
        tables, I = tec_table_of(be, tables, F, T, tint)
        Nd, Nm = int(delays[2]), int(tecs[2])
        if int(tables.shape[0]) != tec_table_doubles(F, Nd, Nm):
            raise ValueError(f"tables of {int(tables.shape[0])} values do not belong to this cube and these axes")
        rounds, (wj, wm) = int(rounds), (int(v) for v in window)
        if not 1 <= rounds <= 4 or not (0 <= wj <= TEC_MAX_DELAYS and 0 <= wm <= TEC_MAX_CELLS):
            raise ValueError("rounds must be in 1 .. 4 and window a pair of cell counts >= 0")
        scalars = fringe_solve_scalars(min_count, min_coh2, refant, niter, tol, A)
        warm = int(sol is not None)
        sol = fringe_sol(be, sol, I, A, vis) if warm else be.empty((I, A, 4), be.f64, vis)
        peaks, info = be.empty((B, I, TEC_PEAK), be.f64, vis), be.empty((I, A), be.f64, vis)
        stats = be.empty(8, be.f64, vis)
        self._call(be, "tecfit", B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, *scalars, warm, sol,
                   peaks, info, stats)
        return sol, peaks, info, stats

    def apply_tec(self, sol, tables, vis, a1, a2, tint, *, inverse=True, weights=None, out=None, weights_out=None):
        """Apply a delay and TEC solution to a [B, T, F] cube (gridhip_apply_tec[_dev]).  inverse=True corrects data: vis
        conj(D) with D = g_p conj(g_q) exp(2 pi i ((tau_p - tau_q) a_f + (tec_p - tec_q) c_f)); inverse=False corrupts a
        model: vis D.  Weights, non-finite rows, out and weights_out, in place and a table of another tint: as
        Context.apply_fringe.  Only the head, a_f and c_f of the table are read: a table of any search axes over the same
        freq, ntime and tint."""
        be = backend(vis)
        nant = int(sol.shape[1]) if hasattr(sol, "shape") and len(sol.shape) == 3 else 0
        B, T, F, A, vis, _, wt, a1, a2 = fringe_cube(be, vis, None, weights, a1, a2, nant)
        tables, I = tec_table_of(be, tables, F, T, tint)
        sol = fringe_sol(be, sol, I, A, vis)
        out = result_array(be, out, be.c128, (B, T, F), "out", vis)
        weights_out = result_array(be, weights_out, be.f64, (B, T, F), "weights_out", vis)
        self._call(be, "apply_tec", B, T, F, A, I, tables, sol, a1, a2, int(bool(inverse)), vis, wt, out, weights_out)
        return out, weights_out

    def dft_predict(self, uvw, comps, x=None, count=None, vis_sub=None, out=None, terms=1, stats=False):
        """The exact visibilities of a component list (gridhip_dft_predict[_dev]; include/gridhip.h, "direct-Fourier
        prediction"): sum_c S_c(x) E_c(u, v) exp(-2 pi i (u l_c + v m_c + w (n_c - 1))), or vis_sub minus that.  uvw
        (wavelengths, not mirrored): a (u, v, w) tuple - w may be None: 0 - or an (n, 3) array; comps: a (C, 10) array of
        rows {l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0} (gridhip.components, Context.components_from_image); x: the n
        fractional frequency offsets the spectral terms are evaluated at (None: 0), terms: how many of f0..f3 are read;
        count: one int64 element (for numpy also an int) - only the first min(max(count, 0), C) rows are used, which
        takes a list built on the device without reading its length back.  out: the array to write (may be vis_sub
        itself); a new one when None.  numpy in gives numpy out; torch cuda tensors take the device form on torch's
        stream.  Returns out, or with stats=True (out, stats), stats the 4 values [components used, components skipped,
        visibilities with non-finite coordinates, slices].  The same bits on every run."""
        be = backend(comps)
        C_, comps = component_list(be, comps)
        u, v, w, st = baselines(be, uvw, 3)
        n, T = int(u.shape[0]), int(terms)
        if not 1 <= T <= 4:
            raise ValueError("terms must be in 1..4")
        x = stream_array(be, x, be.f64, n, "x")
        sub = stream_array(be, vis_sub, be.c128, n, "vis_sub")
        count = component_count(be, count, comps)
        out = result_array(be, out, be.c128, (n,), "out", comps)
        st4 = be.empty(4, be.f64, comps) if stats else None
        self._call(be, "dft_predict", C_, comps, count, T, n, u, v, w, st, x, sub, out, st4)
        return (out, st4) if stats else out

    def phase_shift(self, uvw, vis, R, coords=True, out=None, stats=False):
        """`vis` and its baselines rotated to another phase centre (gridhip_phase_shift[_dev]; include/gridhip.h, "phase
        shift and averaging"): vis * exp(+2 pi i (u l0 + v m0 + w (n0 - 1))) with (l0, m0, n0) the third row of the 3 x 3
        rotation R (rotation_to, rotation_radec; host values whichever back end), and (u', v', w') = R (u, v, w).  uvw
        (wavelengths, not mirrored): a (u, v, w) tuple - w may be None: 0 - or an (n, 3) array.  out: the array to write,
        which may be `vis` itself; a new one when None.  Returns (out, uvw_out) - uvw_out a new (n, 3) array - or with
        coords=False out alone; with stats=True the 4 values [shifted, visibilities with non-finite coordinates (they
        pass through unchanged), 0, 0] are appended.  numpy in gives numpy out; torch cuda tensors take the device form on
        torch's stream and stay on the device."""
        be = backend(vis)
        u, v, w, st = baselines(be, uvw, 3)
        n = int(u.shape[0])
        vis = stream_array(be, vis, be.c128, n, "vis")
        Rp, keep = _rotation(R)
        if Rp is None:
            raise ValueError("R must be a 3 x 3 rotation")
        out = result_array(be, out, be.c128, (n,), "out", vis)
        new = be.empty((n, 3), be.f64, vis) if coords else None
        cols = (new[:, 0], new[:, 1], new[:, 2]) if coords else (None, None, None)
        st4 = be.empty(4, be.f64, vis) if stats else None
        self._call(be, "phase_shift", n, Rp, u, v, w, st, vis, out, *cols, 3, st4)
        res = (out, new) if coords else (out,)
        res = res + (st4,) if stats else res
        return res if len(res) > 1 else res[0]

    def average(self, uvw, vis, group, G, weights=None, x=None, R=None, counts=False, stats=False):
        """The stream collapsed into G weighted samples, one per group (gridhip_average[_dev]; include/gridhip.h, "phase
        shift and averaging").  uvw as for phase_shift; group: the group of every visibility in [0, G) (a sample whose
        group is outside is left out), as average_groups or flag_groups return it with G; None: one group.  weights: n data
        weights (None: ones; a value that is not > 0 flags its sample); x: a further per-sample column averaged the same
        way (dft_predict's fractional frequency, a time), or None.  R: a rotation as for phase_shift - the stream is
        shifted first, with the bits of phase_shift followed by average and without writing the shifted stream.
        Returns (uvw_g (G, 3), vis_g, weights_g, x_g) - x_g None without x - then, with counts=True, the participants of
        every group (int64) and, with stats=True, the 8 values [groups with a participant, participants, flagged, left
        out, not finite, largest group, non-finite coordinates seen by the shift, 0].  A group without participants is
        all zeros with the weight +0.0.  The sums are exact integer sums: the same bits on every run and for any order of
        the stream.  numpy in gives numpy out; torch cuda tensors take the device form on torch's stream: nothing is read
        back."""
        be = backend(vis)
        u, v, w, st = baselines(be, uvw, 3)
        n = int(u.shape[0])
        vis = stream_array(be, vis, be.c128, n, "vis")
        G, group = group_ids(be, group, G, n)
        wt = stream_array(be, weights, be.f64, n, "weights")
        x = stream_array(be, x, be.f64, n, "x")
        Rp, keep = _rotation(R)
        uvw_g = be.empty((G, 3), be.f64, vis)
        vis_g, wt_g = be.empty((G,), be.c128, vis), be.empty((G,), be.f64, vis)
        x_g = None if x is None else be.empty((G,), be.f64, vis)
        cnt = be.empty((G,), be.i64, vis) if counts else None
        st8 = be.empty(8, be.f64, vis) if stats else None
        self._call(be, "average", n, G, group, Rp, u, v, w, st, x, vis, wt, uvw_g[:, 0], uvw_g[:, 1], uvw_g[:, 2], 3, x_g,
                   vis_g, wt_g, cnt, st8)
        return (uvw_g, vis_g, wt_g, x_g) + ((cnt,) if counts else ()) + ((st8,) if stats else ())

    def mosaic(self, facets, theta_src, R, theta_dst, N_dst, kind="cubic", weights=None, window=None, normalize=True,
               wmin=0.0, blank=float("nan"), wsum=False, stats=False, out=None):
        """F images on F tangent planes brought onto one plane and combined (gridhip_mosaic[_dev]; include/gridhip.h,
        "reprojection and mosaicking").  facets: (F, Ns, Ns) float64, all with the field of view theta_src; R: one
        rotation per facet, (F, 3, 3) or (F, 9), from the destination frame to the facet's frame - what phase_shift was
        given to make that facet (facet_grid returns them).  The result is N_dst x N_dst with the field of view theta_dst.
        kind: "nearest", "bilinear" or "cubic" (Keys, a = -1/2).  weights: None, or an array of the facets' shape (a
        primary-beam power, an inverse variance); a sample whose weight is not finite or not > 0 is left out.  window:
        (inner, outer) in facet cells from the facet's centre - 1 inside inner, 0 from outer on, a smoothstep between, per
        axis - or None for inner = outer = Ns / 2: every cell whose footprint lies inside the facet takes part (for
        "nearest", up to half a cell short of that on the low side of an even Ns).  normalize: out = num / den, else num;
        a cell with den <= wmin or beyond the horizon gets `blank`.  A host R is checked here (ValueError); a cuda R is
        judged on the device, where a facet with a bad R is counted and left out.  Returns out, then with wsum=True the
        weight sum of every cell and with stats=True the 8 values [cells covered, cells blank, facets used, facets
        refused, samples left out for a tap that is not finite, most facets on one cell, 0, 0].  numpy in gives numpy
        out; cuda tensors take the device form on torch's stream: nothing is read back, and the call can be captured.
        The same bits on every run."""
        be = backend(facets)
        args = mosaic_args(be, facets, theta_src, R, theta_dst, N_dst, kind, weights, window, normalize, wmin, blank, wsum,
                           stats, out)
        self._call(be, "mosaic", *args)
        res = (args[14],) + ((args[15],) if wsum else ()) + ((args[16],) if stats else ())
        return res if len(res) > 1 else res[0]

    def reproject(self, image, theta_src, R, theta_dst, N_dst, kind="cubic", window=None, blank=float("nan"), out=None):
        """One Ns x Ns image on the tangent plane R away from the destination's, resampled onto the destination plane
        (gridhip_reproject[_dev]): mosaic with one facet, no weights, normalize=True.  R: the 3 x 3 rotation from the
        destination frame to the image's frame.  A model on the full plane becomes facet f's model with R_f.T:
        reproject(model, theta, R_f.T, theta_f, N_f), which Imager.predict takes."""
        be = backend(image)
        if len(getattr(image, "shape", ())) != 2:
            raise ValueError("image must be one Ns x Ns image")
        a = mosaic_args(be, image, theta_src, R, theta_dst, N_dst, kind, None, window, True, 0.0, blank, False, False, out)
        self._call(be, "reproject", a[1], a[2], a[3], a[5], a[6], a[7], a[8], a[11], a[12], a[13], a[14])
        return a[14]

    def components_from_image(self, theta, lam, model, max_components, out=None):
        """The non-zero cells of a model image as a component list (gridhip_components_from_image[_dev]): model is N x N,
        N = image_size(theta, lam), or (T, N, N) Taylor-term planes as mfclean leaves them; every cell where some term is
        not zero becomes a point component at l = theta (x - N/2) / N, m = theta (y - N/2) / N, in row-major order, the
        same list on every run.  Returns (comps, count): comps a (max_components, 10) array whose first min(count,
        max_components) rows are written (out: the array to write; a new one of zeros when None), count the number
        found - an int for numpy, one int64 cuda element for torch tensors, which dft_predict takes as `count` with
        nothing read back."""
        be = backend(model)
        N, max_c = self.image_size(theta, lam), int(max_components)
        T, model = model_planes(be, model, N)
        if max_c < 0:
            raise ValueError("max_components must be >= 0")
        if out is None:
            out = be.zeros((max_c, COMP_DOUBLES), be.f64, model)
        else:
            out = result_array(be, out, be.f64, (max_c, COMP_DOUBLES), "out", model)
        count = be.zeros(1, be.i64, model)
        self._call(be, "components_from_image", float(theta), int(lam), T, model, max_c, out, count)
        return out, (int(count[0]) if be is HOST else count)

    def find_sources(self, theta, lam, image, beam=None, noise=None, border=0, thr=(0, 0), nsigma=(5, 2.5), peak_frac=0,
                     min_cells=1, correct=True, max_sources=1024, out=None, info=True, deblend=0):
        """A catalogue of the N x N float64 map `image`, N = image_size(theta, lam) (gridhip_find_sources[_dev];
        include/gridhip.h, "source finding"): the islands of automask's levels - above T_lo = max(thr[1], nsigma[1] * sigma,
        peak_frac * peak) around at least `min_cells` connected cells above T_hi, no growing - each measured by its moments
        about its peak and written as one component row {l, m, flux, 0, 0, 0, bmaj, bmin, bpa, 0} that dft_predict takes as
        it is, in ascending order of the island's first cell.  `beam` (the 8 values of fit_beam, or None) turns units per
        beam into integrated flux and is deconvolved from the shape; `correct` undoes the cut of a Gaussian at T_lo; an
        island whose deconvolved shape is not positive definite is a point.  `noise` is sigma as for automask.  Returns
        (comps, count, info, stats): comps a (max_sources, 10) array whose first min(count, max_sources) rows are written
        (out: the array to write; a new one of zeros when None); count the islands found - an int for numpy, one int64 cuda
        element for torch tensors, which dft_predict takes as `count`; info (None with info=False) the (max_sources, 16) rows
        [label, ncells, yp, xp, peak, S, Sx, Sy, Sxx, Sxy, Syy, y0, y1, x0, x1, flags (1 point, 2 at the edge, 4 beam
        unusable, 8 = SOURCE_BLENDED)]; stats = [T_hi, T_lo, peak, islands found, rows written, of them points, their
        summed flux, reason].
        deblend = r in 1 .. 32 sets the option "sources_deblend" for this call and puts it back afterwards (0 leaves the
        option as it is): an island with several peaks - local maxima above T_hi that no higher cell of the island lies
        within r cells of - becomes one row per peak, in ascending order of the peaks' cells, each measured over the cells
        that climb to it; the rows of one island share its label and carry flag 8, and count and the stats count rows.
        numpy arrays take the synchronous host form; torch cuda tensors the asynchronous one: nothing is read back, and
        with `noise` a device element the call can be captured."""
        be = backend(image)
        N = self.image_size(theta, lam)
        image = image_of(be, image, (N, N), "image")
        args = source_args(be, thr, nsigma, noise, peak_frac, min_cells, beam, correct, max_sources, out, info, image)
        _deblended(self, deblend, lambda: self._call(be, "find_sources", float(theta), int(lam), image, int(border), *args))
        comps, table, count, stats = args[-4:]
        return comps, (int(count[0]) if be is HOST else count), table, stats

    def imager(self, theta, lam, uvw, imgfn, a1=None, a2=None, weighting="uniform", robust=0.0, taper=0.0, weights=None):
        """Bind the baselines `uvw` (torch cuda tensors, wavelengths, not mirrored: a (u, v, w) tuple or an (n, 3) tensor)
        and the imaging function `imgfn` (predict's tuples; "aw" with the antenna indices a1, a2) once
        (gridhip_imager): mirror, weights, w-bins, kernel tables, both binnings and the PSF are made here.  Returns an
        Imager whose cycle(vis, model) is do_imaging(predict(model, vis_sub=vis))'s image in one asynchronous call.  Every
        argument may be freed or changed afterwards.
        imgfn ("wstack", dict(wstep=, planes=, qpx=, npixFF=, npixKern=)) gives an imager that owns a stack on each of the
        two streams: its psf, pmax and cycle are do_imaging's and its predict is predict's with that tuple (2 Re of the
        layers' sum over pmax, no Hermitian fill), and every other method works as for the other kinds.
        imgfn ("idg", dict(wstep=, planes=, subgrid=, margin=)) gives the same imager with image-domain layers; it needs every
        visibility it keeps on the grid of both streams (u and -u: the library refuses a stream that is not).
        weighting "natural" | "uniform" | "briggs", robust, taper and weights (n cuda float64 data weights in the order of
        vis, or None) are Context.weights' (gridhip_imager_create[_aw]_weighted_dev): the density is taken on the mirrored
        baselines, a visibility whose data weight is not > 0 contributes nothing to any image even where its vis is NaN,
        and the default is the uniform weighting of do_imaging."""
        be = device()
        u, v, w, st = baselines(be, uvw, 3)
        tl, n, h = (float(theta), int(lam)), int(u.shape[0]), C.c_void_p()
        wargs = _weighting(be, weighting, robust, taper, weights, n)
        if wargs == (1, 0.0, 0.0, None):
            name, wargs = "imager_create", ()
        else:
            name = "imager_create_weighted"
        if imgfn[0] == "aw":
            tables, a1, a2 = aw_tables(be, imgfn[1], imgfn[2], imgfn[3], a1, a2)
            self._call(be, name.replace("create", "create_aw"), *tl, *tables, n, u, v, w, st, a1, a2, *wargs, C.byref(h))
        else:
            self._call(be, name, *imaging_function(be, imgfn), *tl, n, u, v, w, st, *wargs, C.byref(h))
        return Imager(self, h, n, self.image_size(theta, lam), u.device)


    def wstack(self, theta, lam, uvw, kernops):
        """Bind the stream `uvw` (torch cuda tensors, wavelengths, taken as given: no mirror, no weights) for w-stacking
        (gridhip_wstack; include/gridhip.h, "w-stacking"): kernops = dict(wstep=, planes=, qpx=, npixFF=, npixKern=), planes
        the w-planes per layer.  The stream is cut into layers, each binned once, and the table of the residual
        w-kernels is built here.  kernops may also be a whole tuple ("wstack", kernops) or ("idg", dict(wstep=, planes=,
        subgrid=, margin=)); the latter makes a stack of image-domain layers: a partition by (layer, tile), no table.  Returns a WStack whose image() / predict() are one asynchronous, capturable pass each;
        uvw may be freed or changed afterwards."""
        be = device()
        opts = stack_options(kernops) if isinstance(kernops, tuple) else wstack_options(kernops)
        u, v, w, st = baselines(be, uvw, 3)
        n, h = int(u.shape[0]), C.c_void_p()
        self._call(be, "wstack_create", *opts, float(theta), int(lam), n, u, v, w, st, C.byref(h))
        return WStack(self, h, n, self.image_size(theta, lam), u.device)


class _Bound(Handle):
    """A handle a context made for n device-resident baselines (a plan, an imager): it runs on the context's device
    and stream, reports through the context and takes contiguous cuda tensors only."""

    def __init__(self, ctx, handle, n):
        self.ctx, self._h, self.n = ctx, handle, n

    _lib = property(lambda self: self.ctx._lib)
    _ctx = property(lambda self: self.ctx)

    def _error(self, rc):
        return self.ctx._error(rc)

    def _vis(self, out, like):
        """a visibility output: the caller's, or a new one"""
        return device().empty(self.n, device().c128, like) if out is None else out


class Plan(_Bound):
    """Baselines binned once (gridhip_plan); grid()/degrid() run the tile kernel only."""
    _destroy, _what = "gridhip_plan_destroy", "plan"

    def __init__(self, ctx, handle, n, grid_shape, gcf_shape):
        super().__init__(ctx, handle, n)
        self.grid_shape, self.gcf_shape = grid_shape, gcf_shape

    def _chk(self, gcf, a):
        self._open()
        assert tuple(gcf.shape) == self.gcf_shape and tuple(a.shape) == self.grid_shape
        assert gcf.is_cuda and a.is_cuda and gcf.is_contiguous() and a.is_contiguous()

    def grid(self, gcf, a, v):
        """a += convgrid2 contributions of visibilities v (cuda complex128, length n)"""
        self._chk(gcf, a)
        assert v.shape[0] == self.n and v.is_contiguous()
        self._call(device(), "plan_grid", gcf, v, a)
        return a

    def degrid(self, gcf, a, out=None):
        self._chk(gcf, a)
        out = self._vis(out, a)
        self._call(device(), "plan_degrid", gcf, a, out)
        return out


class AwPlan(_Bound):
    """aw baselines keyed, their kernels built and binned once (gridhip_aw_plan); grid() / degrid() run the tile kernel
    only, with the kernel values captured at creation."""
    _destroy, _what = "gridhip_aw_plan_destroy", "plan"

    def __init__(self, ctx, handle, n, grid_shape):
        super().__init__(ctx, handle, n)
        self.grid_shape = grid_shape

    def _chk(self, a):
        self._open()
        assert tuple(a.shape) == self.grid_shape and a.is_cuda and a.is_contiguous()

    def grid(self, a, v):
        """a += convgrid4 contributions of visibilities v (cuda complex128, length n)"""
        self._chk(a)
        assert v.shape[0] == self.n and v.is_contiguous()
        self._call(device(), "aw_plan_grid", v, a)
        return a

    def degrid(self, a, out=None):
        """degrid4 of the grid a over the plan's baselines (out is overwritten)"""
        self._chk(a)
        out = self._vis(out, a)
        self._call(device(), "aw_plan_degrid", a, out)
        return out


class WStack(_Bound):
    """A stream bound for w-stacking (gridhip_wstack): image() is Re(sum_l S_l ifft_c(G_l)) of the visibilities, predict()
    its exact adjoint; both take contiguous cuda tensors and run on torch's current stream."""
    _destroy, _what = "gridhip_wstack_destroy", "wstack"

    def __init__(self, ctx, handle, n, N, device):
        super().__init__(ctx, handle, n)
        self.N, self.device = N, device

    def _info(self, i):
        self._open()
        out = [C.c_int64() for _ in range(4)]
        self._check(self._lib.gridhip_wstack_info(self._h, *(C.byref(x) for x in out)))
        return out[i].value

    layers = property(lambda self: self._info(0), doc="the layers L of the stream's w range")
    occupied = property(lambda self: self._info(1), doc="the layers that hold a visibility")
    pmin = property(lambda self: self._info(2), doc="the lowest w-plane, round(w / wstep), of the stream")
    dropped = property(lambda self: self._info(3), doc="visibilities without a finite w, or dropped by the gridder")

    def image(self, vis, out=None):
        """Re(D) of the visibilities `vis` (cuda complex128, length n) -> N x N cuda float64 (out, or a new tensor)"""
        self._open()
        be = device()
        Imager._ok(vis, be.c128, (self.n,), "vis")
        if out is None:
            out = be.empty((self.N, self.N), be.f64, self.device)
        else:
            Imager._ok(out, be.f64, (self.N, self.N), "out")
        self._call(be, "wstack_image", vis, out)
        return out

    def predict(self, model, vis_sub=None, out=None):
        """The stack's prediction of the N x N cuda float64 `model`, or vis_sub minus it; out may be vis_sub."""
        self._open()
        be = device()
        Imager._ok(model, be.f64, (self.N, self.N), "model")
        if vis_sub is not None:
            Imager._ok(vis_sub, be.c128, (self.n,), "vis_sub")
        if out is None:
            out = self._vis(None, self.device)
        else:
            Imager._ok(out, be.c128, (self.n,), "out")
        self._call(be, "wstack_predict", model, vis_sub, out)
        return out


class Imager(_Bound):
    """The baselines of a major cycle bound once (gridhip_imager): cycle() is predict + do_imaging without anything that
    depends on the baselines alone; psf and pmax were computed at creation.  An imager made with ("wstack", kernops)
    runs every pass on layered grids (do_imaging's and predict's "wstack" forms are the two calls it replaces); the
    context option "wstack_middle" selects between the two ways its cycle passes from the prediction to the gridding."""
    _destroy, _what = "gridhip_imager_destroy", "imager"

    def __init__(self, ctx, handle, n, N, device):
        super().__init__(ctx, handle, n)
        self.N, self.device = N, device
        self._psf = None
        self.nterms = 0  # the Taylor terms of set_spectral (0: none)

    @staticmethod
    def _ok(t, dt, shape, what):
        if not (device().ok(t, dt) and tuple(t.shape) == shape):
            raise ValueError(f"{what} must be a contiguous cuda {dt} tensor of shape {shape}")
        return t

    def _pmax(self, psf):
        self._open()
        pm = C.c_double()
        self._check(self._lib.gridhip_imager_psf_dev(self._h, Context._ptr(psf), C.byref(pm)))
        return pm.value

    @property
    def psf(self):
        """do_imaging's psf for these baselines (N x N cuda float64, normalised by pmax)"""
        if self._psf is None:
            self._open()
            self.ctx._use_torch_stream()
            psf = device().empty((self.N, self.N), device().f64, self.device)
            self._pmax(psf)
            self._psf = psf
        return self._psf

    @property
    def pmax(self):
        return self._pmax(None)

    def cycle(self, vis, model=None, out=None, vis_res=None):
        """The image of do_imaging(vis - predict(model)) (of do_imaging(vis) without a model), asynchronous on torch's
        stream.  out: the N x N cuda float64 tensor to write (a new one when None).  vis_res: a length-n cuda complex128
        tensor that receives vis - predict(model); it may be vis itself."""
        self._open()
        be = device()
        self._ok(vis, be.c128, (self.n,), "vis")
        if model is not None:
            self._ok(model, be.f64, (self.N, self.N), "model")
        if vis_res is not None:
            self._ok(vis_res, be.c128, (self.n,), "vis_res")
        if out is None:
            out = be.empty((self.N, self.N), be.f64, self.device)
        else:
            self._ok(out, be.f64, (self.N, self.N), "out")
        self._call(be, "imager_cycle", model, vis, out, vis_res)
        return out

    def predict(self, model, vis_sub=None, out=None):
        """Context.predict for the imager's baselines: the prediction of `model`, or vis_sub minus it; out may be vis_sub."""
        self._open()
        be = device()
        self._ok(model, be.f64, (self.N, self.N), "model")
        if vis_sub is not None:
            self._ok(vis_sub, be.c128, (self.n,), "vis_sub")
        if out is None:
            out = self._vis(None, self.device)
        else:
            self._ok(out, be.c128, (self.n,), "out")
        self._call(be, "imager_predict", model, vis_sub, out)
        return out


    def image_stats(self, image, mask=None, border=0):
        """Context.image_stats of an N x N cuda float64 image with the imager's own scratch
        (gridhip_imager_image_stats_dev): asynchronous, and capturable after a first call."""
        self._open()
        be, NN = device(), (self.N, self.N)
        self._ok(image, be.f64, NN, "image")
        mask = mask_of(be, mask, NN)
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_image_stats", image, mask, int(border), stats)
        return stats

    def automask(self, image, mask=None, noise=None, border=0, absolute=False, thr=(0, 0), nsigma=(5, 2.5), peak_frac=0,
                 min_cells=1, grow=0):
        """Context.automask of an N x N cuda float64 image with the imager's own scratch (gridhip_imager_automask_dev):
        asynchronous, and capturable after a first call.  Returns (mask, stats)."""
        self._open()
        be, NN = device(), (self.N, self.N)
        self._ok(image, be.f64, NN, "image")
        args = automask_args(be, absolute, thr, nsigma, noise, peak_frac, min_cells, grow, self.device)
        mask, m8 = mask_in_place(be, mask, NN, self.device)
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_automask", image, m8, int(border), *args, stats)
        return mask, stats

    def automask_local(self, image, mask=None, border=0, step=16, half=None, kappa=3.0, nclip=3, min_count=16,
                       nsigma=(5, 2.5), min_cells=1, grow=0, absolute=False):
        """Context.automask_local of an N x N cuda float64 image: the context's noise_map(mode="snr"), then this imager's
        automask on the S/N image.  Returns (mask, automask's stats, the S/N image, noise_map's stats)."""
        self._open()
        self._ok(image, device().f64, (self.N, self.N), "image")
        _, _, snr, _, nstats = self._ctx.noise_map(image, mask=mask, exclude=mask is not None, border=border, step=step,
                                                   half=half, kappa=kappa, nclip=nclip, min_count=min_count, mode="snr",
                                                   maps=False)
        mask, astats = self.automask(snr, mask=mask, border=border, absolute=absolute, thr=nsigma, nsigma=(0, 0),
                                     min_cells=min_cells, grow=grow)
        return mask, astats, snr, nstats

    def find_sources(self, image, beam=None, noise=None, border=0, thr=(0, 0), nsigma=(5, 2.5), peak_frac=0, min_cells=1,
                     correct=True, max_sources=1024, out=None, info=True, deblend=0):
        """Context.find_sources of an N x N cuda float64 map with the imager's theta, lam and its own scratch
        (gridhip_imager_find_sources_dev): asynchronous, and capturable after a first call with as many rows.  deblend:
        the context's option "sources_deblend" for this call, as for Context.find_sources.  Returns (comps, count, info,
        stats)."""
        self._open()
        be, NN = device(), (self.N, self.N)
        self._ok(image, be.f64, NN, "image")
        args = source_args(be, thr, nsigma, noise, peak_frac, min_cells, beam, correct, max_sources, out, info, self.device)
        _deblended(self._ctx, deblend, lambda: self._call(be, "imager_find_sources", image, int(border), *args))
        return args[-4], args[-2], args[-3], args[-1]

    def clean(self, image, model=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0, mask=None, nsigma=0.0,
              noise=None, peak_frac=0.0):
        """Context.clean with the imager's own PSF (gridhip_imager_clean_dev): `image` (N x N cuda float64, a cycle's
        output) is updated in place and returned as the residual, `model` (zeros when None) is accumulated into.
        Returns (model, residual, stats); asynchronous, and capturable after a first call.  mask, nsigma, noise,
        peak_frac: as for Context.clean (gridhip_imager_clean_auto_dev, 8 stats); to stay capturable `noise` must be a
        device element such as image_stats(...)[3:4], not a Python number."""
        self._open()
        be, NN = device(), (self.N, self.N)
        image = in_place(be, image, NN, "image")
        model = in_place(be, model, NN, "model", self.device)
        auto = auto_args(be, mask, nsigma, noise, peak_frac, NN, self.device)
        stats = be.empty(8 if auto else 4, be.f64, self.device)
        if auto:
            self._call(be, "imager_clean_auto", image, model, *clean_scalars(gain, threshold, niter, border, patch), *auto,
                       stats)
        else:
            self._call(be, "imager_clean", image, model, *clean_scalars(gain, threshold, niter, border, patch), stats)
        return model, image, stats

    def msclean(self, image, scales, bias=None, model=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0,
                mask=None, nsigma=0.0, noise=None, peak_frac=0.0):
        """Context.msclean with the imager's own PSF (gridhip_imager_msclean_dev).  The imager keeps the cross-PSFs of
        the scale list between calls: a second call with the same `scales` builds and allocates nothing.  Returns
        (model, residual, stats[12]); asynchronous, and capturable after a first call with these scales.  mask, nsigma,
        noise, peak_frac: as for Context.msclean (gridhip_imager_msclean_auto_dev, 16 stats); `noise` as a device element
        to stay capturable."""
        self._open()
        be, NN = device(), (self.N, self.N)
        image = in_place(be, image, NN, "image")
        sc, keep = scale_list(scales, bias)
        model = in_place(be, model, NN, "model", self.device)
        auto = auto_args(be, mask, nsigma, noise, peak_frac, NN, self.device)
        stats = be.empty(16 if auto else 12, be.f64, self.device)
        if auto:
            self._call(be, "imager_msclean_auto", image, model, *sc, *clean_scalars(gain, threshold, niter, border, patch),
                       *auto, stats)
        else:
            self._call(be, "imager_msclean", image, model, *sc, *clean_scalars(gain, threshold, niter, border, patch),
                       stats)
        del keep
        return model, image, stats

    def deconvolve(self, vis, nmajor, model=None, out=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0,
                   scales=None, bias=None, mask=None, nsigma=0.0, peak_frac=0.0, automask=None):
        """Visibilities to a model image in one asynchronous call (gridhip_imager_deconvolve_dev): nmajor times
        image = cycle(vis, model) then clean(image, model), and one closing cycle, so that the returned image is
        do_imaging(vis - predict(model))'s for the returned model.  model (zeros when None) is accumulated into, out
        (a new image when None) receives the closing residual image.  Returns (model, image, stats[nmajor, 4]).
        With `scales` (and optionally `bias`) the minor cycle is msclean (gridhip_imager_msdeconvolve_dev) and stats is
        [nmajor, 12].
        With any of `mask`, `nsigma`, `peak_frac` every major cycle measures its image (image_stats over the whole
        search region) and its minor cycle is clean / msclean under the mask, stopping at max(threshold, nsigma * that
        cycle's sigma, peak_frac * its first peak) (gridhip_imager_[ms]deconvolve_auto_dev): returns (model, image,
        stats[nmajor, 8 | 16], istats[nmajor, 8]).
        With `automask` = dict(absolute=, thr=, nsigma=, peak_frac=, min_cells=, grow=) (Context.automask's keywords and
        defaults; {} takes them all) every major cycle also extends the mask from the image it is about to clean, at that
        cycle's sigma, before its minor cycle (gridhip_imager_[ms]deconvolve_automask_dev): `mask` (zeros when None) is
        the starting mask, UPDATED IN PLACE, and the call returns (model, image, stats[nmajor, 8 | 16], istats[nmajor,
        8], mask, astats[nmajor, 8])."""
        self._open()
        be, NN = device(), (self.N, self.N)
        self._ok(vis, be.c128, (self.n,), "vis")
        model = in_place(be, model, NN, "model", self.device)
        out = be.empty(NN, be.f64, self.device) if out is None else in_place(be, out, NN, "out")
        if int(nmajor) < 0:
            raise ValueError("nmajor must be >= 0")
        if automask is not None:
            if scales is None and bias is not None:
                raise ValueError("bias goes with scales")
            unknown = set(automask) - {"absolute", "thr", "nsigma", "peak_frac", "min_cells", "grow"}
            if unknown:
                raise ValueError(f"automask has no option {sorted(unknown)}")
            am = automask_args(be, automask.get("absolute", False), automask.get("thr", (0, 0)),
                               automask.get("nsigma", (5, 2.5)), None, automask.get("peak_frac", 0),
                               automask.get("min_cells", 1), automask.get("grow", 0), self.device, own_noise=True)
            nsigma, peak_frac = float(nsigma), float(peak_frac)
            if not (nsigma >= 0.0 and nsigma < float("inf")) or not 0.0 <= peak_frac < 1.0:
                raise ValueError("nsigma must be finite and >= 0 and peak_frac in [0, 1)")
            mask, m8 = mask_in_place(be, mask, NN, self.device)
            rows = int(nmajor)
            istats, astats = be.empty((rows, 8), be.f64, self.device), be.empty((rows, 8), be.f64, self.device)
            sc, keep = scale_list(scales, bias) if scales is not None else ((), None)
            stats = be.empty((rows, 16 if sc else 8), be.f64, self.device)
            self._call(be, "imager_msdeconvolve_automask" if sc else "imager_deconvolve_automask", vis, model, out, rows, *sc,
                       *clean_scalars(gain, threshold, niter, border, patch), m8, nsigma, peak_frac, *am, stats, istats,
                       astats)
            del keep
            return model, out, stats, istats, mask, astats
        if mask is not None or nsigma or peak_frac:
            if scales is None and bias is not None:
                raise ValueError("bias goes with scales")
            mask, nsigma, _, peak_frac = auto_args(be, mask, nsigma, None, peak_frac, NN, self.device, own_noise=True)
            istats = be.empty((int(nmajor), 8), be.f64, self.device)
            sc, keep = scale_list(scales, bias) if scales is not None else ((), None)
            stats = be.empty((int(nmajor), 16 if sc else 8), be.f64, self.device)
            self._call(be, "imager_msdeconvolve_auto" if sc else "imager_deconvolve_auto", vis, model, out, int(nmajor), *sc,
                       *clean_scalars(gain, threshold, niter, border, patch), mask, nsigma, peak_frac, stats, istats)
            del keep
            return model, out, stats, istats
        if scales is None:
            if bias is not None:
                raise ValueError("bias goes with scales")
            stats = be.empty((int(nmajor), 4), be.f64, self.device)
            self._call(be, "imager_deconvolve", vis, model, out, int(nmajor),
                       *clean_scalars(gain, threshold, niter, border, patch), stats)
            return model, out, stats
        sc, keep = scale_list(scales, bias)
        stats = be.empty((int(nmajor), 12), be.f64, self.device)
        self._call(be, "imager_msdeconvolve", vis, model, out, int(nmajor), *sc,
                   *clean_scalars(gain, threshold, niter, border, patch), stats)
        del keep
        return model, out, stats

    # -- wide-band imaging (include/gridhip.h, "wide-band imaging") -------------------------------------------------------
    def _terms(self, *stacks):
        """T of the stacks a wide-band call takes: set_spectral's, or - on an imager without terms, which the library
        then refuses - that of the first stack given (1 when there is none)"""
        for t in stacks:
            if self.nterms == 0 and t is not None and len(getattr(t, "shape", ())) == 3:
                return int(t.shape[0])
        return self.nterms or 1

    def set_spectral(self, x, nterms=2):
        """Give the imager `nterms` Taylor terms (1 to 4; gridhip_imager_set_spectral_dev): x holds (nu_k - nu_0) / nu_0
        per visibility (n cuda float64 values in the order of vis; copied).  A visibility whose x is not finite is
        treated as flagged.  Builds and keeps the 2 nterms - 1 spectral PSFs; may synchronise, as creation does."""
        self._open()
        be = device()
        if not 1 <= int(nterms) <= 4:
            raise ValueError("nterms must be 1 to 4")
        if not is_torch(x):
            raise ValueError("x must be a cuda tensor")
        x = be.cv(x, be.f64)
        if tuple(x.shape) != (self.n,):
            raise ValueError(f"x must hold one value per visibility ({self.n}), not {tuple(x.shape)}")
        self.nterms = 0
        self._call(be, "imager_set_spectral", int(nterms), x)
        self.nterms = int(nterms)

    def spectral_psfs(self):
        """The 2T - 1 spectral PSFs set_spectral built ([2T - 1, N, N] cuda float64; [0] is the imager's own PSF)"""
        self._open()
        be = device()
        out = be.empty((2 * self._terms() - 1, self.N, self.N), be.f64, self.device)
        self._call(be, "imager_spectral_psfs", out)
        return out

    def mfs_cycle(self, vis, models=None, out=None, vis_res=None):
        """One wide-band major-cycle step (gridhip_imager_mfs_cycle_dev): with r = vis - sum_q x^q predict(models[q])
        (r = vis without models), out[t] = cycle(x^t r) for the T terms.  models and out are [T, N, N] cuda float64 (out:
        a new one when None); vis_res (length n, may be vis itself) receives r.  Asynchronous on torch's stream."""
        self._open()
        be = device()
        TNN = (self._terms(models, out), self.N, self.N)
        self._ok(vis, be.c128, (self.n,), "vis")
        if models is not None:
            self._ok(models, be.f64, TNN, "models")
        if vis_res is not None:
            self._ok(vis_res, be.c128, (self.n,), "vis_res")
        if out is None:
            out = be.empty(TNN, be.f64, self.device)
        else:
            self._ok(out, be.f64, TNN, "out")
        self._call(be, "imager_mfs_cycle", models, vis, out, vis_res)
        return out

    def mfclean(self, images, models=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0):
        """Context.mfclean with the imager's own spectral PSFs (gridhip_imager_mfclean_dev): `images` ([T, N, N] cuda
        float64, an mfs_cycle's output) is updated in place and returned as the residuals, `models` (zeros when None) is
        accumulated into.  Returns (models, residuals, stats[8]); asynchronous, and capturable after a first call."""
        self._open()
        be = device()
        TNN = (self._terms(images, models), self.N, self.N)
        images = in_place(be, images, TNN, "images")
        models = in_place(be, models, TNN, "models", self.device)
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_mfclean", images, models, *clean_scalars(gain, threshold, niter, border, patch), stats)
        return models, images, stats

    def mfdeconvolve(self, vis, nmajor, models=None, out=None, gain=0.1, threshold=0.0, niter=100, border=0, patch=0):
        """Visibilities to T model images in one asynchronous call (gridhip_imager_mfdeconvolve_dev): nmajor times
        images = mfs_cycle(vis, models) then mfclean(images, models), and one closing mfs_cycle.  models (zeros when
        None) is accumulated into, out (new when None) receives the closing residual images.  Returns (models, images,
        stats[nmajor, 8])."""
        self._open()
        be = device()
        TNN = (self._terms(models, out), self.N, self.N)
        self._ok(vis, be.c128, (self.n,), "vis")
        models = in_place(be, models, TNN, "models", self.device)
        out = be.empty(TNN, be.f64, self.device) if out is None else in_place(be, out, TNN, "out")
        if int(nmajor) < 0:
            raise ValueError("nmajor must be >= 0")
        stats = be.empty((int(nmajor), 8), be.f64, self.device)
        self._call(be, "imager_mfdeconvolve", vis, models, out, int(nmajor),
                   *clean_scalars(gain, threshold, niter, border, patch), stats)
        return models, out, stats

    def selfcal(self, model, vis, a1, a2, nant, *, slot=None, nslots=1, weights=None, phase_only=False, refant=0,
                niter=50, tol=1e-8, gains=None, out=None, weights_out=None):
        """One self-calibration step (gridhip_imager_selfcal_dev): predict(model), Context.gaincal of `vis` against it
        and Context.apply_gains(inverse=True) of vis and weights, as one asynchronous chain that copies nothing and,
        after a first call, can be captured into a graph.  a1, a2 (for an aw imager too), slot, weights, gains, out and
        weights_out are cuda tensors as in those calls; out may be vis and weights_out may be weights.  Returns (gains,
        vis_cal, wt_cal, stats): vis_cal goes into cycle or deconvolve, wt_cal is what a re-weighted imager is created
        with."""
        self._open()
        be = device()
        self._ok(model, be.f64, (self.N, self.N), "model")
        self._ok(vis, be.c128, (self.n,), "vis")
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, nant, slot, nslots, weights)
        mode, refant, warm, niter, tol, gains = solve_args(be, phase_only, refant, niter, tol, gains, A, T, self.device)
        out = result_array(be, out, be.c128, (n,), "out", self.device)
        weights_out = result_array(be, weights_out, be.f64, (n,), "weights_out", self.device)
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_selfcal", model, vis, A, T, a1, a2, slot, wt, mode, refant, warm, niter, tol, gains, out,
                   weights_out, stats)
        return gains, out, weights_out, stats

    def peel(self, model, vis, model_vis, a1, a2, nant, *, slot=None, nslots=1, weights=None, phase_only=False, refant=0,
             niter=50, tol=1e-8, gains=None, out=None, weights_out=None):
        """One peel step (gridhip_imager_peel_dev): predict(model) into row 0 of `model_vis` - a contiguous (D, n)
        complex128 cuda tensor whose rows 1 .. D - 1 hold the caller's models of the bright directions, for instance
        Context.dft_predict of their components - then Context.ddcal of `vis` against all D rows, Context.dd_subtract of
        the directions 1 .. D - 1 and Context.apply_gains(gains[0], inverse=True) of the result and the weights, as one
        asynchronous chain that copies nothing and, after a first call, can be captured into a graph.  The other
        arguments are selfcal's; gains is (D, nslots, nant).  Returns (gains, vis_cal, wt_cal, stats)."""
        self._open()
        be = device()
        self._ok(model, be.f64, (self.N, self.N), "model")
        self._ok(vis, be.c128, (self.n,), "vis")
        n, A, T, a1, a2, slot, vis, wt = gain_stream(be, vis, a1, a2, nant, slot, nslots, weights)
        if not (is_torch(model_vis) and len(model_vis.shape) == 2 and be.ok(model_vis, be.c128)):
            raise ValueError("model_vis must be a contiguous cuda complex128 tensor of shape (D, n): its row 0 is written")
        D, model_vis = model_rows(be, model_vis, n)
        mode, refant, warm, niter, tol, gains = solve_args(be, phase_only, refant, niter, tol, gains, A, T, self.device, D)
        out = result_array(be, out, be.c128, (n,), "out", self.device)
        weights_out = result_array(be, weights_out, be.f64, (n,), "weights_out", self.device)
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_peel", model, vis, A, T, D, a1, a2, slot, wt, mode, refant, warm, niter, tol, model_vis,
                   gains, out, weights_out, stats)
        return gains, out, weights_out, stats

    def flag(self, model, vis, group=None, G=None, weights=None, nsigma=5.0, amax=0.0, min_count=8, niter=3, out=None):
        """Context.flag_residuals of `vis` against the imager's own prediction of `model` (gridhip_imager_flag_dev):
        predict(model) and the flagging as one asynchronous chain that copies nothing and, after a first call of a
        shape, can be captured into a graph.  group, weights and out are cuda tensors as in that call; out may be weights.
        Returns (weights, flags, group_stats, stats): the weights go into Context.imager(weights=...) or selfcal."""
        self._open()
        be = device()
        self._ok(model, be.f64, (self.N, self.N), "model")
        self._ok(vis, be.c128, (self.n,), "vis")
        n, G, group, vis, _, wt = flag_stream(be, vis, None, group, G, weights, self.n)
        scalars = flag_scalars(nsigma, amax, min_count, niter)
        out, flags, gstats, stats = flag_outputs(be, n, G, out, self.device)
        self._call(be, "imager_flag", model, vis, G, group, wt, *scalars, out, flags, gstats, stats)
        return out, flags, gstats, stats

    def weight_stats(self):
        """The stats of the weighting the imager was created with (gridhip_imager_weight_stats_dev): Context.weights'
        8 values as a cuda tensor, copied on torch's stream."""
        self._open()
        be = device()
        stats = be.empty(8, be.f64, self.device)
        self._call(be, "imager_weight_stats", stats)
        return stats

    def beam(self, window=8, cut=0.5):
        """Context.fit_beam on the imager's own PSF (gridhip_imager_beam_dev): the 8 values as a cuda tensor,
        asynchronous."""
        self._open()
        be = device()
        beam = be.empty(8, be.f64, self.device)
        self._call(be, "imager_beam", int(window), float(cut), beam)
        return beam

    def restore(self, model, residual, support=None, window=8, cut=0.5, out=None):
        """The restored image of a deconvolve's or a clean's (model, residual) with the beam fitted to the imager's own
        PSF (gridhip_imager_restore_dev): returns (restored, beam), the image in units per beam and the 8 values of the
        fit, both on the device.  With an explicit `support` (1 to 32) the call is asynchronous and, after a first
        call, capturable together with deconvolve.  support=None fits the beam first and READS IT BACK to derive the
        support (Context.restore): one synchronisation, and a ValueError when the fit failed or the beam needs more
        than 32 cells.  out may be `residual` itself."""
        self._open()
        be, NN = device(), (self.N, self.N)
        self._ok(model, be.f64, NN, "model")
        self._ok(residual, be.f64, NN, "residual")
        out = be.empty(NN, be.f64, self.device) if out is None else in_place(be, out, NN, "out")
        if support is None:
            support = beam_support(self.beam(window, cut).tolist())
        beam = be.empty(8, be.f64, self.device)
        self._call(be, "imager_restore", model, residual, int(window), float(cut), int(support), out, beam)
        return out, beam


_default = {}


def components(l, m, flux, spectral=None, fwhm=None, pa=None):
    """Pack a component list for Context.dft_predict: l, m (direction cosines) and flux are C values each; spectral: a
    (C, k) array, k <= 3, of the further polynomial coefficients f1..fk of S(x) = f0 + x (f1 + x (f2 + x f3)); fwhm: a
    (C, 2) array of the Gaussian FWHM axes (bmaj, bmin) in direction cosines, None or 0: points; pa: C position angles in
    radians from +m towards +l.  numpy in gives a (C, 10) float64 ndarray, torch tensors a tensor on l's device."""
    be = backend(l)
    l = be.cv(l, be.f64).reshape(-1)
    n = int(l.shape[0])
    out = be.zeros((n, COMP_DOUBLES), be.f64, l)
    out[:, 0], out[:, 1], out[:, 2] = l, be.cv(m, be.f64).reshape(-1), be.cv(flux, be.f64).reshape(-1)
    if spectral is not None:
        sp = be.cv(spectral, be.f64).reshape(n, -1)
        if sp.shape[1] > 3:
            raise ValueError("spectral holds at most the three coefficients f1, f2, f3 per component")
        out[:, 3:3 + sp.shape[1]] = sp
    if fwhm is not None:
        out[:, 6:8] = be.cv(fwhm, be.f64).reshape(n, 2)
    if pa is not None:
        out[:, 8] = be.cv(pa, be.f64).reshape(-1)
    return out


def ddcal_lds_antennas(D):
    """The most antennas whose gains and sums of one interval Context.ddcal's iteration kernel keeps in LDS for D
    directions (gridhip_ddcal_lds_antennas): more antennas add to global memory directly.  0 for D outside 1..8."""
    return int(_lib.load().gridhip_ddcal_lds_antennas(int(D)))


def jonescal_lds_antennas():
    """The most antennas whose Jones matrices and sums of one interval Context.jonescal's iteration kernel keeps in LDS
    (gridhip_jonescal_lds_antennas): more antennas add to global memory directly."""
    return int(_lib.load().gridhip_jonescal_lds_antennas())


def flag_groups(a1, a2, slot=None, by="baseline"):
    """The groups Context.flag_residuals clips within, from the antenna pair (and the solution interval) of every
    visibility: by "baseline" - one group per unordered antenna pair; "slot" - per interval; "baseline_slot" - per pair
    and interval; "all" - one group.  Returns (group, G): compact int64 ids in [0, G), numbered in the order of the
    sorted (pair, slot) keys, and their number.  torch tensors (any device) or anything numpy converts; plumbing - torch
    operations only, no kernel of the library - and G is read back: one synchronisation where the tensors are on a device."""
    import torch
    if by not in ("baseline", "slot", "baseline_slot", "all"):
        raise ValueError(f'by must be "baseline", "slot", "baseline_slot" or "all", not {by!r}')
    a1, a2 = (torch.as_tensor(x).to(torch.int64).reshape(-1) for x in (a1, a2))
    if a1.shape != a2.shape:
        raise ValueError("a1 and a2 must hold one antenna per visibility each")
    if by in ("slot", "baseline_slot"):
        if slot is None:
            raise ValueError(f'by="{by}" needs slot')
        slot = torch.as_tensor(slot).to(torch.int64).reshape(-1).to(a1.device)
        if slot.shape != a1.shape:
            raise ValueError("slot must hold one interval per visibility")
    if by == "all" or a1.numel() == 0:
        return torch.zeros_like(a1), 1
    lo, hi = torch.minimum(a1, a2), torch.maximum(a1, a2)
    cols = {"baseline": (lo, hi), "slot": (slot,), "baseline_slot": (lo, hi, slot)}[by]
    _, group = torch.unique(torch.stack(cols, dim=1), dim=0, sorted=True, return_inverse=True)
    return group.to(torch.int64), int(group.max()) + 1


def sumthreshold_tile():
    """(tile_t, tile_f): the tile of time steps x channels that a work-group of Context.sumthreshold's stage kernel owns
    (gridhip_sumthreshold_tile)."""
    tt, tf = C.c_int64(), C.c_int64()
    rc = _lib.load().gridhip_sumthreshold_tile(C.byref(tt), C.byref(tf))
    if rc != 0:
        raise GridHipError(rc, "gridhip_sumthreshold_tile")
    return tt.value, tf.value


def waterfall_layout(a1, a2, time, ntime, chan, nchan, order="btf"):
    """Where every sample of a flat visibility stream lies in the cube Context.sumthreshold takes, from its antenna pair,
    its integer time index in [0, ntime) and its integer channel in [0, nchan).  Returns (index, B, pairs): index (int64)
    is the cell of every sample in the flattened cube - [B][ntime][nchan] for order "btf", [ntime][B][nchan] for "tbf" -
    so that cube.view(-1)[index] = stream fills the cube and weights.view(-1)[index] is the way back; B is the number of
    baselines, the unordered antenna pairs numbered in sorted order as in flag_groups; pairs (B, 2) holds their antennas.
    A cube of weights starts from zeros: the cells nobody fills keep the weight 0 and are flagged on input.  torch
    tensors (any device) or anything numpy converts; plumbing - torch operations only, no kernel of the library - and B
    is read back: one synchronisation where the tensors are on a device."""
    import torch
    if order not in ("btf", "tbf"):
        raise ValueError(f'order must be "btf" or "tbf", not {order!r}')
    a1, a2, time, chan = (torch.as_tensor(x).to(torch.int64).reshape(-1) for x in (a1, a2, time, chan))
    dev = a1.device
    a2, time, chan = a2.to(dev), time.to(dev), chan.to(dev)
    ntime, nchan = int(ntime), int(nchan)
    if not (a1.shape == a2.shape == time.shape == chan.shape):
        raise ValueError("a1, a2, time and chan must hold one value per visibility each")
    if ntime < 1 or nchan < 1:
        raise ValueError("ntime and nchan must be >= 1")
    if a1.numel() == 0:
        return torch.zeros_like(a1), 1, torch.zeros((1, 2), dtype=torch.int64, device=dev)
    if bool(((time < 0) | (time >= ntime) | (chan < 0) | (chan >= nchan)).any()):
        raise ValueError("time must lie in [0, ntime) and chan in [0, nchan)")
    lo, hi = torch.minimum(a1, a2), torch.maximum(a1, a2)
    pairs, b = torch.unique(torch.stack((lo, hi), dim=1), dim=0, sorted=True, return_inverse=True)
    B = int(pairs.shape[0])
    index = ((b * ntime + time) if order == "btf" else (time * B + b)) * nchan + chan
    return index.to(torch.int64), B, pairs.contiguous()


def rm_tile():
    """(LOS per work-group, depths per work-group, channels of a chunk) of Context.rmsynth's kernel (gridhip_rm_tile)."""
    out = (C.c_int64 * 3)()
    rc = _lib.load().gridhip_rm_tile(out)
    if rc != 0:
        raise GridHipError(rc, "gridhip_rm_tile")
    return int(out[0]), int(out[1]), int(out[2])


def noise_grid(N, border=0, step=16):
    """The node centres of Context.noise_map's mesh for an N x N image (gridhip_noise_map_nodes): G int64 cell indices,
    the same along y and x."""
    import numpy as np
    G = int(_lib.load().gridhip_noise_map_nodes(int(N), int(border), int(step)))
    if G < 0:
        raise GridHipError(G, "gridhip_noise_map_nodes")
    M = int(N) - 2 * int(border)
    return int(border) + np.minimum(np.arange(G, dtype=np.int64) * int(step) + int(step) // 2, M - 1)


def contsub_tile():
    """(rows per work-group, channels per staged chunk) of Context.contsub's kernel for axis=-1 (gridhip_contsub_tile)."""
    out = (C.c_int64 * 2)()
    rc = _lib.load().gridhip_contsub_tile(out)
    if rc != 0:
        raise GridHipError(rc, "gridhip_contsub_tile")
    return int(out[0]), int(out[1])


def fringe_tile():
    """(delays per work-group, channels per staged chunk, rates per lane-pass) of Context.fringe_search's kernel
    (gridhip_fringe_tile)."""
    out = (C.c_int64 * 3)()
    rc = _lib.load().gridhip_fringe_tile(out)
    if rc != 0:
        raise GridHipError(rc, "gridhip_fringe_tile")
    return int(out[0]), int(out[1]), int(out[2])


def fringe_grid(freq, time, tint, pad=4):
    """The delay and rate cells a band and a solution interval support: returns (tau0, dtau, Nd), (r0, drate, Nr), both
    centred on 0 (cell N // 2 is zero).  dtau = 1 / (pad * F * median channel step) with Nd = pad * F cells, so that the
    axis spans the unambiguous range 1 / step at `pad` cells per resolution element; the rate axis is built the same way
    from the tint time steps of an interval (0: all) and the median time step.  Pure host code: Context.fringe_tables
    takes the two triples."""
    import numpy as np
    freq, time = np.asarray(freq, dtype=np.float64).reshape(-1), np.asarray(time, dtype=np.float64).reshape(-1)
    F, T, pad = freq.size, time.size, int(pad)
    if F < 1 or T < 1 or pad < 1:
        raise ValueError("freq and time must hold at least one value each and pad must be >= 1")
    tint, _ = fringe_intervals(T, tint)
    df = float(np.median(np.abs(np.diff(freq)))) if F > 1 else 1.0
    dt = float(np.median(np.abs(np.diff(time)))) if T > 1 else 1.0
    if not (np.isfinite(df) and df > 0.0 and np.isfinite(dt) and dt > 0.0):
        raise ValueError("the median channel step and time step must be finite and > 0")
    Nd, Nr = pad * F, pad * tint
    if Nd > FRINGE_MAX_DELAYS or Nr > FRINGE_MAX_RATES:
        raise ValueError(f"pad * F = {Nd} delays (at most {FRINGE_MAX_DELAYS}) or pad * tint = {Nr} rates (at most "
                         f"{FRINGE_MAX_RATES}): lower pad")
    dtau, drate = 1.0 / (pad * F * df), 1.0 / (pad * tint * dt)
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nr // 2) * drate, drate, Nr)


def tec_tile():
    """(delays per work-group tile, TEC cells per tile, channels per staged chunk) of Context.tec_search's kernel
    (gridhip_tec_tile)."""
    out = (C.c_int64 * 3)()
    rc = _lib.load().gridhip_tec_tile(out)
    if rc != 0:
        raise GridHipError(rc, "gridhip_tec_tile")
    return int(out[0]), int(out[1]), int(out[2])


def tec_coordinates(freq):
    """(a_f, c_f, s, nu0) of include/gridhip.h, "dispersive delay (TEC) calibration", in plain numpy: a_f = nu_f - nu0, the
    orthogonalised dispersive coordinate c_f = z_f - s a_f with z_f = -kappa (1 / nu_f - 1 / nu0), and the slope s that was
    taken out.  Host code for choosing a grid; the table's own values are made on the device."""
    import numpy as np
    freq = np.asarray(freq, dtype=np.float64).reshape(-1)
    if freq.size < 1 or not (np.isfinite(freq).all() and (freq > 0.0).all()):
        raise ValueError("freq must hold at least one channel, every one finite and > 0")
    nu0 = freq[0] + 0.5 * (freq[-1] - freq[0])
    a, z = freq - nu0, -(TEC_KAPPA * (1.0 / freq - 1.0 / nu0))
    den = float((a * a).sum())
    s = float((a * z).sum()) / den if den > 0.0 else 0.0
    return a, z - s * a, s, nu0


def tec_grid(freq, tec_max, pad=4):
    """The delay and TEC cells a band supports: returns (tau0, dtau, Nd), (tec0, dtec, Nm), both centred on 0.  The delay
    axis is gridhip.fringe_grid's: Nd = pad * F cells of 1 / (pad * F * median channel step).  dtec = 1 / (pad * (max c_f -
    min c_f)) TEC units - `pad` cells per resolution element of the orthogonalised dispersive coordinate - and Nm = 2 *
    ceil(tec_max / dtec) + 1 cells, enough for |tec| <= tec_max.  Pure host code: Context.tec_tables takes the two triples."""
    import math
    import numpy as np
    freq, pad, tec_max = np.asarray(freq, dtype=np.float64).reshape(-1), int(pad), float(tec_max)
    F = freq.size
    _, c, _, _ = tec_coordinates(freq)
    if pad < 1 or not (math.isfinite(tec_max) and tec_max >= 0.0):
        raise ValueError("pad must be >= 1 and tec_max finite and >= 0")
    df = float(np.median(np.abs(np.diff(freq)))) if F > 1 else 1.0
    span = float(c.max() - c.min())
    if not (np.isfinite(df) and df > 0.0 and np.isfinite(span) and span > 0.0):
        raise ValueError("the band must hold at least three distinct channels: it has no dispersive curvature otherwise")
    Nd, dtau, dtec = pad * F, 1.0 / (pad * F * df), 1.0 / (pad * span)
    Nm = 2 * int(math.ceil(tec_max / dtec)) + 1
    if Nd > TEC_MAX_DELAYS or Nm > TEC_MAX_CELLS:
        raise ValueError(f"pad * F = {Nd} delays (at most {TEC_MAX_DELAYS}) or {Nm} TEC cells (at most {TEC_MAX_CELLS}): "
                         f"lower pad or tec_max")
    return (-(Nd // 2) * dtau, dtau, Nd), (-(Nm // 2) * dtec, dtec, Nm)


def tec_clock(sol, tables):
    """The non-dispersive (clock) delays of a delay-TEC solution: tau_clock = tau_eff - s * tec, [I, nant], with s from the
    head of the table.  Host code: numpy in and out (copy a cuda solution and at least the table's head to the host first)."""
    import numpy as np
    sol, head = np.asarray(sol, dtype=np.float64), np.asarray(tables[:TEC_HEAD], dtype=np.float64)
    if sol.ndim != 3 or sol.shape[2] != 4 or head.shape != (TEC_HEAD,) or head[0] != 1.0:
        raise ValueError("sol must be [I, nant, 4] and tables a valid table of Context.tec_tables")
    return sol[:, :, 0] - head[12] * sol[:, :, 1]


def channel_coordinate(freq):
    """The channel coordinate Context.contsub fits in: x = (f - mid) / half with mid = 0.5 * (fmin + fmax) and half =
    0.5 * (fmax - fmin), so that the band maps onto [-1, 1], where the Chebyshev basis is well conditioned; all zeros for one
    channel or equal frequencies.  Pure host code: a float64 ndarray."""
    import numpy as np
    f = np.asarray(freq, dtype=np.float64).reshape(-1)
    if f.size == 0:
        raise ValueError("freq must hold at least one channel")
    mid, half = 0.5 * (f.min() + f.max()), 0.5 * (f.max() - f.min())
    if not half > 0.0:
        return np.zeros_like(f)
    return (f - mid) / half


def faraday_grid(lam2, oversample=4, phi_max=None):
    """The Faraday depths a set of channels supports (Brentjens & de Bruyn 2005, eqs. 61-63), from their squared
    wavelengths lam2 (at least two different ones): returns (phi0, dphi, J, fwhm, max_scale, phi_limit) with
    fwhm = 2 sqrt(3) / (max lam2 - min lam2), the width of the RMSF; dphi = fwhm / oversample; phi_limit =
    sqrt(3) / max |delta lam2| over neighbours of the sorted channels, the depth at which the widest channel gap loses
    half its sensitivity; max_scale = pi / min lam2, the widest structure in depth that is seen; J = 2 floor(phi_max /
    dphi) + 1 depths (phi_max None: phi_limit), at most 511; phi0 = -(J - 1) / 2 * dphi, so that depth 0 is on the grid.
    Pure host code: Context.rm_tables takes phi = (phi0, dphi, J) and fwhm."""
    import math
    import numpy as np
    lam2 = np.sort(np.asarray(lam2, dtype=np.float64).reshape(-1))
    if lam2.size < 2 or not np.isfinite(lam2).all() or not lam2[0] > 0.0 or not lam2[-1] > lam2[0]:
        raise ValueError("lam2 must hold at least two different finite squared wavelengths > 0")
    oversample = float(oversample)
    if not (math.isfinite(oversample) and oversample > 0.0):
        raise ValueError("oversample must be finite and > 0")
    fwhm = 2.0 * math.sqrt(3.0) / float(lam2[-1] - lam2[0])
    dphi = fwhm / oversample
    phi_limit = math.sqrt(3.0) / float(np.max(np.abs(np.diff(lam2))))
    max_scale = math.pi / float(lam2[0])
    phi_max = phi_limit if phi_max is None else float(phi_max)
    if not (math.isfinite(phi_max) and phi_max >= 0.0):
        raise ValueError("phi_max must be finite and >= 0")
    J = min(2 * int(math.floor(phi_max / dphi)) + 1, 511)
    return -(J - 1) / 2 * dphi, dphi, J, fwhm, max_scale, phi_limit


def rotation_to(l0, m0):
    """The minimal rotation that takes the w-axis to the direction cosines (l0, m0) - what Context.phase_shift and
    Context.average take as R: a (3, 3) float64 ndarray whose third row is (l0, m0, n0), n0 = sqrt(1 - l0^2 - m0^2), and
    which turns about the axis perpendicular to the old and the new centre (no field rotation).  Plumbing: numpy only."""
    import math
    import numpy as np
    l0, m0 = float(l0), float(m0)
    r2 = l0 * l0 + m0 * m0
    if not r2 < 1.0:
        raise ValueError("l0^2 + m0^2 must be below 1: the new centre lies in front of the old one")
    n0 = math.sqrt(1.0 - r2)
    k = 1.0 / (1.0 + n0)
    return np.array([[1.0 - k * l0 * l0, -k * l0 * m0, -l0], [-k * l0 * m0, 1.0 - k * m0 * m0, -m0], [l0, m0, n0]])


def facet_grid(theta, nf, overlap=0.0, N=1):
    """nf x nf facets that tile the field of view `theta`: returns (centres, R, theta_f, window).  centres: (F, 2), the
    (l0, m0) of facet f = j * nf + i at l0 = theta ((i + 1/2) / nf - 1/2), m0 likewise from j; R: (F, 9), rotation_to of
    every centre - what Context.phase_shift takes to make the facet and Context.mosaic to bring it back; theta_f =
    (theta / nf) (1 + overlap), the field of view of every facet; window: (inner, outer) in cells of an N x N facet (N = 1:
    as fractions of the facet's side, to be multiplied by its size) for Context.mosaic.  Neighbouring centres lie
    D = N / (1 + overlap) cells apart and inner + outer = D, so that along a seam the smoothsteps of the two facets sum to 1:
    the feathered facets tile the field without a gap.  The feather takes the inner half of the overlap, outer =
    D / 2 + (N - D) / 4, and leaves the outer half, (N - D) / 4 cells at every edge, to the taps of the interpolation:
    "cubic" needs 2 cells there (overlap = 0 is a hard window that reaches the facet's edge, which only "nearest"
    fills).  Plumbing: numpy only."""
    import numpy as np
    theta, nf, overlap, N = float(theta), int(nf), float(overlap), float(N)
    if not (theta > 0.0 and nf >= 1 and overlap >= 0.0 and N > 0.0):
        raise ValueError("facet_grid needs theta > 0, nf >= 1, overlap >= 0 and N > 0")
    c = theta * ((np.arange(nf) + 0.5) / nf - 0.5)
    centres = np.array([(c[i], c[j]) for j in range(nf) for i in range(nf)], dtype=np.float64).reshape(nf * nf, 2)
    R = np.array([rotation_to(l0, m0).ravel() for l0, m0 in centres]).reshape(nf * nf, 9)
    D = N / (1.0 + overlap)
    outer = D / 2 + (N - D) / 4
    return centres, R, (theta / nf) * (1.0 + overlap), (D - outer, outer)


def rotation_radec(ra0, dec0, ra1, dec1):
    """The rotation from the (u, v, w) frame of the phase centre (ra0, dec0) to that of (ra1, dec1), radians:
    M(ra1, dec1) M(ra0, dec0)^T, M having the rows e_u = (-sin ra, cos ra, 0), e_v = (-sin dec cos ra, -sin dec sin ra,
    cos dec), e_w = (cos dec cos ra, cos dec sin ra, sin dec).  Its third row is the new centre in the old frame:
    l0 = cos dec1 sin(ra1 - ra0).  A (3, 3) float64 ndarray.  Plumbing: numpy only."""
    import numpy as np

    def M(ra, dec):
        sr, cr, sd, cd = np.sin(ra), np.cos(ra), np.sin(dec), np.cos(dec)
        return np.array([[-sr, cr, 0.0], [-sd * cr, -sd * sr, cd], [cd * cr, cd * sr, sd]])
    return M(float(ra1), float(dec1)) @ M(float(ra0), float(dec0)).T


def average_groups(a1, a2, time, ntime=1, chan=None, nchan=1, uvw=None, bda=None):
    """The groups Context.average collapses: one per unordered antenna pair, per window `time // f` of the integer time
    index and per block `chan // nchan` of the integer channel index (chan None: one block).  f = ntime, or with
    bda=max_factor the baseline-dependent f_b = clamp(floor(ntime * Lmax / L_b), ntime, max_factor), L_b the largest
    sqrt(u^2 + v^2) of baseline b in `uvw` (a (u, v, w) tuple or an (n, 3) array) and Lmax the largest L_b: the longest
    baseline keeps ntime, shorter ones average longer.  Returns (group, G, a1_g, a2_g): compact int64 ids in [0, G),
    numbered in the order of the sorted (pair, window, block) keys as in flag_groups, their number, and the antenna pair
    of every group.  torch tensors (any device) or anything numpy converts; plumbing - torch operations only, no kernel of
    the library - and G is read back: one synchronisation where the tensors are on a device."""
    import torch
    a1, a2, time = (torch.as_tensor(x).to(torch.int64).reshape(-1) for x in (a1, a2, time))
    dev = a1.device
    a2, time = a2.to(dev), time.to(dev)
    ntime, nchan = int(ntime), int(nchan)
    if a1.shape != a2.shape or a1.shape != time.shape:
        raise ValueError("a1, a2 and time must hold one value per visibility each")
    if ntime < 1 or nchan < 1:
        raise ValueError("ntime and nchan must be >= 1")
    if chan is None:
        chan = torch.zeros_like(a1)
    else:
        chan = torch.as_tensor(chan).to(torch.int64).reshape(-1).to(dev)
        if chan.shape != a1.shape:
            raise ValueError("chan must hold one channel per visibility")
    if a1.numel() == 0:
        return torch.zeros_like(a1), 1, torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    lo, hi = torch.minimum(a1, a2), torch.maximum(a1, a2)
    if bda is None:
        window = torch.div(time, ntime, rounding_mode="floor")
    else:
        most = int(bda)
        if most < ntime:
            raise ValueError("bda, the largest factor, must be >= ntime")
        if uvw is None:
            raise ValueError("bda needs uvw")
        if isinstance(uvw, (tuple, list)):
            u, v = (torch.as_tensor(c).to(torch.float64).reshape(-1).to(dev) for c in uvw[:2])
        else:
            uvw = torch.as_tensor(uvw).to(torch.float64).to(dev)
            u, v = uvw[:, 0], uvw[:, 1]
        if u.shape != a1.shape or v.shape != a1.shape:
            raise ValueError("uvw must hold one baseline per visibility")
        _, bl = torch.unique(torch.stack((lo, hi), dim=1), dim=0, sorted=True, return_inverse=True)
        length = torch.zeros(int(bl.max()) + 1, dtype=torch.float64, device=dev)
        length = length.scatter_reduce(0, bl, torch.sqrt(u * u + v * v), reduce="amax")
        factor = torch.floor(ntime * length.max() / length)
        factor = torch.where(length > 0, factor, torch.full_like(factor, float(most))).clamp(ntime, most).to(torch.int64)
        window = torch.div(time, factor[bl], rounding_mode="floor")
    block = torch.div(chan, nchan, rounding_mode="floor")
    keys, group = torch.unique(torch.stack((lo, hi, window, block), dim=1), dim=0, sorted=True, return_inverse=True)
    return group.to(torch.int64), int(keys.shape[0]), keys[:, 0].contiguous(), keys[:, 1].contiguous()


def joint_deconvolve(imagers, vis, nmajor, metric="sumsq", weights=None, noise_plane=None, **clean_kw):
    """The joint major cycle over P imagers of one N and one context - one per Stokes parameter, or one per channel - a
    composition DEFINED BY THE CALLS IT REPLACES (include/gridhip.h, "joint deconvolution"):
        repeat nmajor times:
            images[p] = imagers[p].cycle(vis[p], model=models[p], out=images[p])     for every p
            noise = ctx.image_stats(images[noise_plane], border=border)[3:4]          when nsigma > 0
            ctx.jclean(images, psfs, metric, weights, models=models, noise=noise, **clean_kw)
        images[p] = imagers[p].cycle(vis[p], model=models[p], out=images[p])         for every p
    `vis` holds one stream per imager ([P, n], or a sequence of P tensors).  psfs is the stack of the imagers' PSFs,
    built by the first call and kept; where every entry of `imagers` is the same object - the Stokes streams of one set
    of baselines - it is that imager's one PSF.  noise_plane: the plane whose robust sigma the nsigma term multiplies
    (None: the last one, Stokes V of an I, Q, U, V set).  clean_kw: jclean's gain, threshold, niter, border, patch,
    models, mask, nsigma and peak_frac.  Returns (models, images, stats[nmajor, 16]): the models accumulated into, the
    closing residual images and jclean's stats of every major cycle.  Everything is enqueued on torch's stream and
    nothing is read back; after a first call the loop can be captured into a graph."""
    imagers = list(imagers)
    P, nmajor = len(imagers), int(nmajor)
    if not 1 <= P <= JOINT_MAX_PLANES or nmajor < 0:
        raise ValueError(f"joint_deconvolve takes 1 .. {JOINT_MAX_PLANES} imagers and nmajor >= 0")
    first = imagers[0]
    ctx, N, dev = first.ctx, first.N, first.device
    if any(im.ctx is not ctx or im.N != N for im in imagers):
        raise ValueError("the imagers must share one context and one image size")
    if len(vis) != P:
        raise ValueError(f"vis must hold one stream per imager ({P})")
    unknown = set(clean_kw) - {"gain", "threshold", "niter", "border", "patch", "models", "mask", "nsigma", "peak_frac"}
    if unknown:
        raise ValueError(f"joint_deconvolve has no option {sorted(unknown)}")
    kw = dict(clean_kw)
    be = device()
    models = in_place(be, kw.pop("models", None), (P, N, N), "models", dev)
    nsigma, border = float(kw.get("nsigma", 0.0)), int(kw.get("border", 0))
    plane = P - 1 if noise_plane is None else int(noise_plane)
    if not 0 <= plane < P:
        raise ValueError(f"noise_plane must be in 0 .. {P - 1}")
    cached = getattr(first, "_joint_psfs", None)
    if cached is None or len(cached[0]) != P or any(a is not b for a, b in zip(cached[0], imagers)):
        shared = all(im is first for im in imagers)
        psfs = first.psf.reshape(1, N, N) if shared else be.torch.stack([im.psf for im in imagers])
        cached = first._joint_psfs = (tuple(imagers), psfs)
    psfs = cached[1]
    images = be.empty((P, N, N), be.f64, dev)
    stats = be.empty((nmajor, 16), be.f64, dev)
    for i in range(nmajor):
        for p, im in enumerate(imagers):
            im.cycle(vis[p], model=models[p], out=images[p])
        noise = ctx.image_stats(images[plane], border=border)[3:4] if nsigma > 0.0 else None
        stats[i].copy_(ctx.jclean(images, psfs, metric, weights, models=models, noise=noise, **kw)[2])
    for p, im in enumerate(imagers):
        im.cycle(vis[p], model=models[p], out=images[p])
    return models, images, stats


def default_context(device=0):
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]


def _ctx_for(a):
    if is_torch(a):
        return default_context(a.device.index or 0)
    return default_context(0)


def grid(a, p, v):
    return _ctx_for(a).grid(a, p, v)


def convgrid(gcf, a, p, v):
    return _ctx_for(a).convgrid(gcf, a, p, v)


def convgrid2(gcf, a, p, wbin, v):
    return _ctx_for(a).convgrid2(gcf, a, p, wbin, v)


def degrid2(gcf, a, p, wbin, out=None):
    return _ctx_for(a).degrid2(gcf, a, p, wbin, out)
