"""The one marshalling path of the binding: every entry point turns its arguments into what include/gridhip.h takes
through the helpers here, whichever library the arguments come from.

A call picks its back end once, by its leading array (`backend`): HOST for numpy arrays - the synchronous
gridhip_<op> - or the torch one for cuda tensors - the asynchronous gridhip_<op>_dev on torch's current stream.  A
back end knows how to make an argument "contiguous, of dtype complex128 / float64 / int64, or None" without copying
one that already is, how to allocate an output like it and how to take an address; `Handle._call` does the rest,
guided by the prototype table of _lib.py."""
import ctypes as C

import numpy as np

from ._lib import POINTERS, GridHipError


class _Host:
    """numpy arrays -> host pointers"""
    suffix = ""
    c128, f64, i64 = np.complex128, np.float64, np.int64
    form, bad_grid = "a C-contiguous complex128 ndarray", ValueError
    array = "C-contiguous ndarray"  # the kind of array this back end takes, for messages about other dtypes

    @staticmethod
    def cv(x, dt):
        return None if x is None else np.ascontiguousarray(x, dtype=dt)

    @staticmethod
    def empty(shape, dt, like):
        return np.empty(shape, dtype=dt)

    @staticmethod
    def zeros(shape, dt, like):
        return np.zeros(shape, dtype=dt)

    @staticmethod
    def ok(x, dt):
        return isinstance(x, np.ndarray) and x.dtype == dt and x.flags.c_contiguous

    @staticmethod
    def ptr(x):
        return C.c_void_p(x.ctypes.data)

    @staticmethod
    def bind(owner):
        pass


class _Device:
    """torch cuda tensors -> device pointers; the context is first bound to torch's current stream"""
    suffix = "_dev"
    form, bad_grid = "a contiguous cuda complex128 tensor", AssertionError
    array = "contiguous cuda tensor"

    def __init__(self):
        import torch
        self.torch = torch
        self.c128, self.f64, self.i64 = torch.complex128, torch.float64, torch.int64

    @staticmethod
    def cv(x, dt):
        return None if x is None else x.to(dt).contiguous()  # (both return x itself when there is nothing to do)

    def empty(self, shape, dt, like):
        """like: a tensor on the device wanted, or the torch.device itself"""
        return self.torch.empty(shape, dtype=dt, device=getattr(like, "device", like))

    def zeros(self, shape, dt, like):
        return self.torch.zeros(shape, dtype=dt, device=getattr(like, "device", like))

    @staticmethod
    def ok(x, dt):
        return x.is_cuda and x.dtype == dt and x.is_contiguous()

    @staticmethod
    def ptr(x):
        return C.c_void_p(x.data_ptr())

    @staticmethod
    def bind(owner):
        owner._ctx._use_torch_stream()


HOST = _Host()
_device = None


def device():
    """the torch back end (torch is imported when the first tensor arrives)"""
    global _device
    if _device is None:
        _device = _Device()
    return _device


def is_torch(x):
    return type(x).__module__.startswith("torch")


def backend(x):
    """the back end of a call, chosen once by its leading array"""
    return device() if type(x).__module__.startswith("torch") else HOST


def baselines(be, p, k):
    """The first k components (u, v[, w]) of a baseline argument and their element stride (include/gridhip.h,
    uv_stride): a (u, v, w) tuple gives k contiguous float64 vectors at stride 1 - components past k are not touched,
    the gridders take (u, v, None) - and an (n, 3) array gives views of its columns at stride 3."""
    cv, f64 = be.cv, be.f64
    if isinstance(p, (tuple, list)):
        return (cv(p[0], f64), cv(p[1], f64), 1) if k == 2 else (cv(p[0], f64), cv(p[1], f64), cv(p[2], f64), 1)
    if p.ndim == 2 and p.shape[1] == 3:
        m = cv(p, f64)
        return (m[:, 0], m[:, 1], 3) if k == 2 else (m[:, 0], m[:, 1], m[:, 2], 3)
    raise ValueError("p must be a (u, v, w) tuple or an (n, 3) array")


def imaging_function(be, imgfn):
    """("simple",) | ("conv", kv) | ("w_cache", kernops) -> (kind, wstep, Q, npixFF, gh, gw, kv), the leading arguments
    of gridhip_do_imaging, gridhip_predict and gridhip_imager_create_dev.  kernops = dict(wstep=, qpx=, npixFF=,
    npixKern=) as KernelOptions (src/Gridding.hs:30-38); no wstep, or 0: 2000.
    ("wstack", kernops with planes=) -> (4, wstep, qpx, npixFF, npixKern, planes, None) by wstack_options' rules: the
    kind gridhip_imager_create_dev takes for an imager that owns a stack (gridhip_do_imaging and gridhip_predict refuse
    it: they have their _wstack forms).
    ("idg", dict(wstep=, planes=, subgrid=, margin=)) -> (4, wstep, 0, margin, subgrid, planes, None) by idg_options' rules:
    the same kind with image-domain layers, which qpx = 0 selects."""
    if imgfn[0] == "simple":
        return 0, 0, 0, 0, 0, 0, None
    if imgfn[0] == "conv":
        kv = be.cv(imgfn[1], be.c128)
        Q, _, gh, gw = kv.shape
        return 1, 0, Q, 0, gh, gw, kv
    if imgfn[0] == "w_cache":
        ko = imgfn[1]
        side = int(ko["npixKern"])
        return 2, int(ko.get("wstep") or 2000), int(ko["qpx"]), int(ko["npixFF"]), side, side, None
    if imgfn[0] in ("wstack", "idg"):
        wstep, M, Q, ff, S = stack_options(imgfn)
        return 4, wstep, Q, ff, S, M, None
    raise ValueError("unknown imaging function")


def wstack_options(ko):
    """dict(wstep=, planes=, qpx=, npixFF=, npixKern=) -> (wstep, M, qpx, npixFF, npixKern), the leading arguments of the
    w-stacking entry points (include/gridhip.h, "w-stacking"); no wstep, or 0: 2000, as for "w_cache".  What the library
    would refuse is refused here, before any call: wstep or planes below 1, a shape outside the w-kernel shape rule."""
    wstep, M = int(ko.get("wstep") or 2000), int(ko["planes"])
    Q, ff, S = int(ko["qpx"]), int(ko["npixFF"]), int(ko["npixKern"])
    if wstep < 1 or M < 1:
        raise ValueError(f"wstack: wstep ({wstep}) and planes ({M}) must be >= 1")
    if not (ff > 0 and S > 0 and Q > 0 and S <= ff and (ff * Q) // 2 - Q * (S // 2) >= Q - 1):
        raise ValueError(f"wstack: npixFF={ff}, npixKern={S}, qpx={Q} is outside the w-kernel shape rule")
    return wstep, M, Q, ff, S


IDG_SUBGRIDS = (16, 24, 32)


def idg_options(ko):
    """dict(wstep=, planes=, subgrid=, margin=) -> (wstep, M, 0, margin, subgrid), the leading arguments of the w-stacking
    entry points for image-domain layers (include/gridhip.h, "w-stacking", IMAGE-DOMAIN LAYERS): qpx = 0 selects them, npixFF
    carries the margin and npixKern the subgrid; no wstep, or 0: 2000.  What the library would refuse is refused here, before
    any call: wstep or planes below 1, a subgrid other than 16, 24 or 32, a margin that is odd or outside [4, subgrid / 2]."""
    wstep, M = int(ko.get("wstep") or 2000), int(ko["planes"])
    Sg, K = int(ko["subgrid"]), int(ko["margin"])
    if wstep < 1 or M < 1:
        raise ValueError(f"idg: wstep ({wstep}) and planes ({M}) must be >= 1")
    if Sg not in IDG_SUBGRIDS:
        raise ValueError(f"idg: subgrid ({Sg}) must be one of {IDG_SUBGRIDS}")
    if K % 2 or not 4 <= K <= Sg // 2:
        raise ValueError(f"idg: margin ({K}) must be even and in [4, subgrid / 2 = {Sg // 2}]")
    return wstep, M, 0, K, Sg


def stack_options(imgfn):
    """("wstack", kernops) | ("idg", options) -> the five leading arguments of the w-stacking entry points"""
    if imgfn[0] == "idg":
        return idg_options(imgfn[1])
    if imgfn[0] == "wstack":
        return wstack_options(imgfn[1])
    raise ValueError("a stack is made from (\"wstack\", kernops) or (\"idg\", options)")


def idg_trusted(N):
    """The slice of the cells of either axis of an N x N image that image-domain layers fill (8 |x - N div 2| <= 3 N, the
    inner three quarters): image[idg_trusted(N), idg_trusted(N)] is the trusted region, every other cell is exactly 0."""
    N = int(N)
    return slice(N // 2 - (3 * N) // 8, N // 2 + (3 * N) // 8 + 1)


def aw_tables(be, wkernels, wbins, akernels, a1, a2):
    """-> (W, Q, S, A, wkerns, wvals, akerns), a1, a2 as gridhip_aw_imaging and every entry point with its layout take them"""
    wk, wv, ak = be.cv(wkernels, be.c128), be.cv(wbins, be.f64), be.cv(akernels, be.c128)
    W, Q, _, S, _ = wk.shape
    return (W, Q, S, ak.shape[0], wk, wv, ak), be.cv(a1, be.i64), be.cv(a2, be.i64)


def aw_kernels(be, wkerns, akerns, index):
    """-> (W, Q, S, A, wkerns, akerns), (wbin, a1, a2) as gridhip_awgrid, gridhip_awdegrid and gridhip_aw_plan_create_dev
    take the tables and the index triple of convgrid4"""
    wk, ak = be.cv(wkerns, be.c128), be.cv(akerns, be.c128)
    W, Q, _, S, _ = wk.shape
    wbin, a1, a2 = index
    return (W, Q, S, ak.shape[0], wk, ak), (be.cv(wbin, be.i64), be.cv(a1, be.i64), be.cv(a2, be.i64))


def in_place(be, x, shape, what, like=None):
    """An N x N float64 image an entry point updates in place (clean's residual and model, deconvolve's image): the
    caller's own array, which must be in the form the ABI takes - a converted copy would take the update with it - or,
    for None, a new one of zeros on `like`'s device."""
    if x is None and like is not None:
        return be.zeros(shape, be.f64, like)
    if not (be is backend(x) and be.ok(x, be.f64) and tuple(x.shape) == tuple(shape)):
        raise ValueError(f"{what} must be {be.form.replace('complex128', 'float64')} of shape {tuple(shape)}"
                         " (it is updated in place)")
    return x


def clean_scalars(gain, threshold, niter, border, patch):
    """gain, threshold, niter, border, patch as every clean entry point takes them"""
    return float(gain), float(threshold), int(niter), int(border), int(patch)


def mask_of(be, mask, shape):
    """A clean mask as the ABI takes it - N x N bytes, non-zero where a component may be centred - or None: a bool or
    uint8 array of `be`'s own kind and of the image's shape; a bool one is reinterpreted, nothing is converted."""
    if mask is None:
        return None
    if be is not backend(mask) or not hasattr(mask, "dtype"):
        raise ValueError(f"mask must be a {be.array} of dtype bool or uint8")
    u8, b1 = (np.uint8, np.bool_) if be is HOST else (be.torch.uint8, be.torch.bool)
    if mask.dtype not in (u8, b1):
        raise ValueError(f"mask must be of dtype bool or uint8, not {mask.dtype}")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask must be of shape {tuple(shape)}, as the image")
    mask = be.cv(mask, mask.dtype)
    return mask.view(u8) if mask.dtype == b1 else mask


def auto_args(be, mask, nsigma, noise, peak_frac, shape, like, own_noise=False):
    """mask, nsigma, noise, peak_frac as the _auto entry points take them, or None when all four are at their defaults
    (the caller then takes the plain entry point).  noise: sigma as a number, or one float64 element of `be`'s own kind
    (element 3 of an image_stats result: stats[3:4]) - on the device nothing is read back.  A NUMBER with device
    images is uploaded from pageable host memory by this call: a copy that cannot be captured into a graph and that
    makes the call wait for the host - inside a graph, or to stay asynchronous, pass a device element.  own_noise: the entry point
    measures sigma itself (deconvolve)."""
    import math
    if mask is None and not nsigma and noise is None and not peak_frac:
        return None
    nsigma, peak_frac = float(nsigma), float(peak_frac)
    if not (math.isfinite(nsigma) and nsigma >= 0.0):
        raise ValueError("nsigma must be finite and >= 0")
    if not 0.0 <= peak_frac < 1.0:
        raise ValueError("peak_frac must be in [0, 1)")
    mask = mask_of(be, mask, shape)
    if noise is None:
        if nsigma > 0.0 and not own_noise:
            raise ValueError("nsigma > 0 needs noise (sigma, e.g. image_stats(...)[3:4])")
    elif isinstance(noise, (int, float)):
        noise = np.array([noise], dtype=np.float64)
        if be is not HOST:
            noise = be.torch.from_numpy(noise).to(getattr(like, "device", like))
    else:
        if be is not backend(noise) or not be.ok(noise, be.f64) or int(np.prod(tuple(noise.shape))) != 1:
            raise ValueError(f"noise must be a number or a {be.array} of one float64 element")
    return mask, nsigma, noise, peak_frac


def automask_args(be, absolute, thr, nsigma, noise, peak_frac, min_cells, grow, like, own_noise=False):
    """absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, grow as the automask entry points take
    them (include/gridhip.h, "auto-masking").  thr and nsigma are (hi, lo) pairs; a single number stands for both.  noise:
    as for auto_args - a number, or one float64 element of `be`'s own kind such as image_stats(...)[3:4]; a NUMBER with
    device images is uploaded by this call and cannot be captured.  own_noise: the entry point measures sigma itself
    (deconvolve), and noise is left out of the result."""
    import math

    def pair(x, what):
        hi, lo = (x, x) if isinstance(x, (int, float)) else x
        hi, lo = float(hi), float(lo)
        if not (math.isfinite(hi) and math.isfinite(lo) and 0.0 <= lo <= hi):
            raise ValueError(f"{what} must be (hi, lo), finite, with 0 <= lo <= hi")
        return hi, lo
    thr, nsigma, peak_frac = pair(thr, "thr"), pair(nsigma, "nsigma"), float(peak_frac)
    min_cells, grow = int(min_cells), int(grow)
    if not 0.0 <= peak_frac < 1.0:
        raise ValueError("peak_frac must be in [0, 1)")
    if min_cells < 1 or not 0 <= grow <= 32:
        raise ValueError("min_cells must be >= 1 and grow in 0 .. 32")
    head, tail = (int(bool(absolute)), *thr, *nsigma), (peak_frac, min_cells, grow)
    if own_noise:
        return head + tail
    if noise is None:
        if nsigma[0] > 0.0:
            raise ValueError("nsigma > 0 needs noise (sigma, e.g. image_stats(...)[3:4]); pass nsigma=0 for fixed levels")
    elif isinstance(noise, (int, float)):
        noise = np.array([noise], dtype=np.float64)
        if be is not HOST:
            noise = be.torch.from_numpy(noise).to(getattr(like, "device", like))
    elif be is not backend(noise) or not be.ok(noise, be.f64) or int(np.prod(tuple(noise.shape))) != 1:
        raise ValueError(f"noise must be a number or a {be.array} of one float64 element")
    return head + (noise,) + tail


def mask_in_place(be, mask, shape, like):
    """The mask an automask updates in place: the caller's own N x N uint8 or bool array of `be`'s kind in the ABI's form
    (a converted copy would take the update with it), or, for None, a new uint8 one of zeros.  -> (the array the caller
    gets back, its uint8 view for the ABI)"""
    if mask is None:
        u8 = np.uint8 if be is HOST else be.torch.uint8
        mask = be.zeros(shape, u8, like)
        return mask, mask
    if be is backend(mask) and hasattr(mask, "dtype") and not be.ok(mask, mask.dtype):
        raise ValueError(f"mask must be a {be.array} (it is updated in place)")
    return mask, mask_of(be, mask, shape)


def scale_list(scales, bias):
    """S, scales, bias as every msclean entry point takes them: host float64 arrays whichever back end the images come
    from (they fix launch shapes and kernel arguments), passed by address - the caller keeps the returned arrays alive
    for the call.  bias=None: 1 - 0.6 a_s / a_max (1 for the delta alone)."""
    sc = np.ascontiguousarray(scales, dtype=np.float64).ravel()
    if sc.size < 1:
        raise ValueError("scales must hold at least the delta scale 0")
    if bias is None:
        amax = float(sc.max())
        bias = 1.0 - 0.6 * sc / amax if amax > 0.0 else np.ones_like(sc)
    bs = np.ascontiguousarray(bias, dtype=np.float64).ravel()
    if bs.size != sc.size:
        raise ValueError(f"bias must hold one value per scale ({sc.size}), not {bs.size}")
    f64p = C.POINTER(C.c_double)
    return (int(sc.size), sc.ctypes.data_as(f64p), bs.ctypes.data_as(f64p)), (sc, bs)


JOINT_METRICS = {"sum": 0, "sumsq": 1}  # gridhip_jclean's metric
JOINT_MAX_PLANES = 8


def joint_search(metric, weights, P):
    """weights, metric as gridhip_jclean takes them: the metric by name and P host float64 weights whichever back end the
    images come from, passed by address - the caller keeps the returned array alive for the call.  weights=None: 1 / P
    each for "sum" (the mean image, so that thresholds stay in image units), 1 each for "sumsq".  What the library would
    refuse is refused here: a weight that is not finite and >= 0, or none above 0."""
    if metric not in JOINT_METRICS:
        raise ValueError(f"metric must be one of {sorted(JOINT_METRICS)}, not {metric!r}")
    if weights is None:
        w = np.full(P, 1.0 / P if metric == "sum" else 1.0, dtype=np.float64)
    else:
        if is_torch(weights):
            weights = weights.detach().cpu().numpy()
        w = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    if w.size != P:
        raise ValueError(f"weights must hold one value per plane ({P}), not {w.size}")
    if not (np.isfinite(w).all() and (w >= 0.0).all() and (w > 0.0).any()):
        raise ValueError("weights must be finite and >= 0, at least one of them > 0")
    return (w.ctypes.data_as(C.POINTER(C.c_double)), JOINT_METRICS[metric]), w


def psf_planes(be, psfs, P, N):
    """Q, psfs as gridhip_jclean takes the PSFs: (N, N) or (1, N, N) - one PSF for all planes - or (P, N, N), one per
    plane, float64"""
    shape = tuple(getattr(psfs, "shape", ()))
    if shape == (N, N):
        shape = (1, N, N)
    if len(shape) != 3 or shape[1:] != (N, N) or shape[0] not in (1, P):
        raise ValueError(f"psfs must be {(N, N)}, {(1, N, N)} or {(P, N, N)}: one PSF, or one per plane, not {shape}")
    return shape[0], be.cv(psfs, be.f64)


def image_of(be, x, shape, what):
    """An N x N float64 image an entry point only reads (restore's model and residual), converted where it must be"""
    x = be.cv(x, be.f64)
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{what} must be of shape {tuple(shape)}")
    return x


def beam_support(beam):
    """The support a restore needs for the fitted beam `beam` (the 8 values, read back when they are on the device:
    one synchronisation): the smallest R with exp(-lambda_min R^2) <= 1e-9, lambda_min the smaller eigenvalue of
    [[A, B], [B, C]].  Raises when the fit failed or when R exceeds the 32 cells gridhip_restore takes."""
    import math
    A, B, C_, ok = (float(beam[i]) for i in (0, 1, 2, 7))
    lam = 0.5 * (A + C_) - math.hypot(0.5 * (A - C_), B)
    if not (ok != 0.0 and ok == ok and lam > 0.0 and math.isfinite(A + C_)):
        raise ValueError("the beam's fit failed: there is no support to derive (pass support= and a beam of your own)")
    R = max(1, math.ceil(math.sqrt(math.log(1e9) / lam)))
    while R > 1 and math.exp(-lam * (R - 1) ** 2) <= 1e-9:  # (the square root's rounding)
        R -= 1
    if R > 32:
        raise ValueError(f"the beam needs a support of {R} cells, above the 32 gridhip_restore takes: pass support=32 to"
                         " truncate it")
    return R


WEIGHTINGS = {"natural": 0, "uniform": 1, "briggs": 2}


def weighting(be, mode, robust, taper, weights, n):
    """mode, robust, taper_sigma, wt_in as gridhip_weights and the weighted imager creations take them: the mode by name,
    a finite robust, a taper sigma >= 0 in wavelengths (0: none) and the data weights - n float64 values (converted
    where they must be; an array already in the ABI's form goes as it is, so that it can be the output too) or None."""
    import math
    if mode not in WEIGHTINGS:
        raise ValueError(f"weighting must be one of {sorted(WEIGHTINGS)}, not {mode!r}")
    robust, taper = float(robust), float(taper)
    if not math.isfinite(robust):
        raise ValueError("robust must be finite")
    if not taper >= 0.0:
        raise ValueError("taper must be >= 0 (the sigma in wavelengths; 0: no taper)")
    if weights is not None:
        if be is not backend(weights) and be is not HOST:
            raise ValueError(f"weights must be {be.form.replace('complex128', 'float64')}")
        weights = be.cv(weights, be.f64)
        if tuple(weights.shape) != (n,):
            raise ValueError(f"weights must hold one value per visibility ({n}), not {tuple(weights.shape)}")
    return WEIGHTINGS[mode], robust, taper, weights


def _integers(be, x, n, what):
    """an index array as the ABI takes it: n int64 values of `be`'s own kind; other integer widths are converted, any
    other dtype (a float index is a mistake, not a format) and any other length are refused"""
    if be is HOST:
        x = np.asarray(x)
        integral = x.dtype.kind in "iu"
    else:
        integral = is_torch(x) and not (x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == be.torch.bool)
    if not integral:
        raise ValueError(f"{what} must be an integer {be.array}, not {getattr(x, 'dtype', type(x))}")
    if tuple(x.shape) != (n,):
        raise ValueError(f"{what} must hold one index per visibility ({n}), not {tuple(x.shape)}")
    return be.cv(x, be.i64)


def stream_array(be, x, dt, n, what):
    """a per-visibility input: n values converted to dt where they must be, or None"""
    if x is None:
        return None
    if be is not backend(x) and be is not HOST:
        raise ValueError(f"{what} must be a {be.array}")
    if be is HOST:
        x = np.asarray(x)
    if dt is be.f64 and (x.dtype.kind == "c" if be is HOST else x.dtype.is_complex):
        raise ValueError(f"{what} must be real, not {x.dtype}")
    if n < 0:
        n = int(x.shape[0]) if len(x.shape) == 1 else -1
    if tuple(x.shape) != (n,):
        raise ValueError(f"{what} must be one-dimensional with one value per visibility, not of shape {tuple(x.shape)}")
    return be.cv(x, dt)


def result_array(be, x, dt, shape, what, like):
    """an output: the caller's own array in the ABI's form (it is written in place), or a new one"""
    if x is None:
        return be.empty(shape, dt, like)
    if not (be is backend(x) and be.ok(x, dt) and tuple(x.shape) == tuple(shape)):
        raise ValueError(f"{what} must be a {be.array} of shape {tuple(shape)} and the output's dtype (it is written in place)")
    return x


def jones_array(be, x, n, what):
    """a four-correlation stream or a table of Jones matrices as the ABI takes it: (n, 2, 2) complex values (n < 0: any
    number of them), converted to contiguous complex128 where they must be"""
    if x is None or (be is not backend(x) and be is not HOST):
        raise ValueError(f"{what} must be a {be.array}")
    if be is HOST:
        x = np.asarray(x)
    shape = tuple(int(v) for v in x.shape)
    if len(shape) != 3 or shape[1:] != (2, 2) or (n >= 0 and shape[0] != n):
        raise ValueError(f"{what} must be of shape ({'n' if n < 0 else n}, 2, 2): XX, XY, YX, YY per sample, not {shape}")
    return be.cv(x, be.c128)


def gain_stream(be, vis, a1, a2, nant, slot, nslots, weights, jones=False):
    """n, A, T, a1, a2, slot, vis, wt as gridhip_gaincal, gridhip_apply_gains and gridhip_imager_selfcal_dev take the
    visibility stream: slot None goes as NULL and needs nslots == 1.  jones: vis is (n, 2, 2), the four correlations of
    every sample (gridhip_jonescal, gridhip_apply_jones)."""
    # (its length is the stream's: any one-dimensional array)
    vis = jones_array(be, vis, -1, "vis") if jones else stream_array(be, vis, be.c128, -1, "vis")
    n, A, T = int(vis.shape[0]), int(nant), int(nslots)
    if A < 2 or T < 1:
        raise ValueError("nant must be >= 2 and nslots >= 1")
    if slot is None and T != 1:
        raise ValueError("nslots > 1 needs slot, the solution interval of every visibility")
    a1, a2 = _integers(be, a1, n, "a1"), _integers(be, a2, n, "a2")
    slot = None if slot is None else _integers(be, slot, n, "slot")
    return n, A, T, a1, a2, slot, vis, stream_array(be, weights, be.f64, n, "weights")


JONES_MODES = {"full": 0, "diagonal": 1, "phase": 2}  # gridhip_jonescal's mode


def solve_args(be, phase_only, refant, niter, tol, gains, A, T, like, D=None):
    """mode, refant, warm, niter, tol, gains as the solving entry points take them: refant None is -1 (no rotation); gains
    None starts from 1 in a new [T][A] array ([D][T][A] with D, the direction-dependent solves), a given one - in the
    ABI's form: it is updated in place - is the warm start.  D == "jones": phase_only is gridhip_jonescal's mode by name
    and the gains are [T][A][2][2]."""
    import math
    if D == "jones" and phase_only not in JONES_MODES:
        raise ValueError(f"mode must be one of {sorted(JONES_MODES)}, not {phase_only!r}")
    refant = -1 if refant is None else int(refant)
    niter, tol = int(niter), float(tol)
    if refant >= A:
        raise ValueError(f"refant must be below nant ({A}), or None")
    if niter < 0 or not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError("niter must be >= 0 and tol finite and >= 0")
    warm = int(gains is not None)
    shape = (T, A) if D is None else (T, A, 2, 2) if D == "jones" else (D, T, A)
    gains = result_array(be, gains, be.c128, shape, "gains", like)
    return JONES_MODES[phase_only] if D == "jones" else int(bool(phase_only)), refant, warm, niter, tol, gains


STOKES_BITS = {"I": 1, "Q": 2, "U": 4, "V": 8}
STOKES_BASES = {"linear": 0, "circular": 1}


def stokes_args(be, vis, basis, which, inverse, out):
    """n, basis, which, inverse, vis, stokes as gridhip_stokes takes them.  Forward: vis (n, 2, 2) is read and `out`, the
    (4, n) block whose selected rows are written, is the caller's own or a new one of zeros.  Inverse: vis is the (4, n)
    block, all four rows, and `out` the (n, 2, 2) stream to write.  -> (the arguments, the array the caller gets back)"""
    if basis not in STOKES_BASES:
        raise ValueError(f"basis must be one of {sorted(STOKES_BASES)}, not {basis!r}")
    letters = str(which).upper()
    if not letters or any(c not in STOKES_BITS for c in letters) or len(set(letters)) != len(letters):
        raise ValueError(f"which must name some of I, Q, U, V once each, not {which!r}")
    mask = sum(STOKES_BITS[c] for c in letters)
    if inverse:
        if mask != 15:
            raise ValueError("the inverse form reads all four rows: which must be 'IQUV'")
        if vis is None or (be is not backend(vis) and be is not HOST):
            raise ValueError(f"vis must be a {be.array}")
        block = be.cv(np.asarray(vis) if be is HOST else vis, be.c128)
        if len(block.shape) != 2 or int(block.shape[0]) != 4:
            raise ValueError(f"the Stokes block must be of shape (4, n), not {tuple(block.shape)}")
        n = int(block.shape[1])
        out = result_array(be, out, be.c128, (n, 2, 2), "out", block)
        return (n, STOKES_BASES[basis], mask, 1, out, block), out
    vis = jones_array(be, vis, -1, "vis")
    n = int(vis.shape[0])
    out = be.zeros((4, n), be.c128, vis) if out is None else result_array(be, out, be.c128, (4, n), "out", vis)
    return (n, STOKES_BASES[basis], mask, 0, vis, out), out


DD_MAX_DIRECTIONS = 8  # the most directions of gridhip_ddcal


def model_rows(be, x, n):
    """D, model_vis as gridhip_ddcal and gridhip_dd_subtract take the models of the directions: a (D, n) array, or (n,)
    for one direction, converted to contiguous complex128 where it must be"""
    if x is None or (be is not backend(x) and be is not HOST):
        raise ValueError(f"model_vis must be a {be.array}")
    if be is HOST:
        x = np.asarray(x)
    shape = tuple(int(v) for v in x.shape)
    shape = (1,) + shape if len(shape) == 1 else shape
    if len(shape) != 2 or (n >= 0 and shape[1] != n) or not 1 <= shape[0] <= DD_MAX_DIRECTIONS:
        raise ValueError(f"model_vis must be of shape (D, n) with D in 1..{DD_MAX_DIRECTIONS} and one column per "
                         f"visibility, not {tuple(x.shape)}")
    return shape[0], be.cv(x, be.c128)


def direction_mask(directions, D):
    """dirs as gridhip_dd_subtract takes a set of directions: None is all D of them"""
    if directions is None:
        return (1 << D) - 1
    mask = 0
    for d in directions:
        d = int(d)
        if not 0 <= d < D:
            raise ValueError(f"a direction must be in 0..{D - 1}, not {d}")
        mask |= 1 << d
    return mask


FLAG_MAX_ROUNDS = 16  # the most clipping rounds of gridhip_flag_residuals


def flag_stream(be, vis, model_vis, group, G, weights, n=-1):
    """n, G, group, vis, model_vis, wt_in as gridhip_flag_residuals and gridhip_imager_flag_dev take the stream: group None
    goes as NULL and needs G in (None, 1); a given group needs G, the number of groups (gridhip.flag_groups returns both)."""
    vis = stream_array(be, vis, be.c128, n, "vis")
    n = int(vis.shape[0])
    if group is None:
        if G not in (None, 1):
            raise ValueError("G > 1 needs group, the group of every visibility")
        G = 1
    else:
        if G is None:
            raise ValueError("group needs G, the number of groups (flag_groups returns both)")
        group = _integers(be, group, n, "group")
    G = int(G)
    if G < 1:
        raise ValueError("G must be >= 1")
    return (n, G, group, vis, stream_array(be, model_vis, be.c128, n, "model_vis"),
            stream_array(be, weights, be.f64, n, "weights"))


def flag_scalars(nsigma, amax, min_count, niter):
    """nsigma, amax, min_count, niter as the flagging entry points take them"""
    import math
    nsigma, amax, min_count, niter = float(nsigma), float(amax), int(min_count), int(niter)
    if not (math.isfinite(nsigma) and nsigma > 0.0):
        raise ValueError("nsigma must be finite and > 0")
    if not amax >= 0.0:
        raise ValueError("amax must be >= 0 (0: no limit)")
    if min_count < 1 or not 0 <= niter <= FLAG_MAX_ROUNDS:
        raise ValueError(f"min_count must be >= 1 and niter in 0 .. {FLAG_MAX_ROUNDS}")
    return nsigma, amax, min_count, niter


def flag_outputs(be, n, G, out, like):
    """wt_out, flags_out, group_stats, stats: new arrays, or for wt_out the caller's own (it may be `weights` itself)"""
    u8 = np.uint8 if be is HOST else be.torch.uint8
    return (result_array(be, out, be.f64, (n,), "out", like), be.empty((n,), u8, like), be.empty((G, 4), be.f64, like),
            be.empty((8,), be.f64, like))


ST_MAX_STAGES, ST_MAX_ROUNDS = 7, 4  # the most stages (windows up to 64) and rounds of gridhip_sumthreshold


def cube_arrays(be, vis, model_vis, weights, order):
    """B, T, F, order, vis, model_vis, wt_in as gridhip_sumthreshold takes a cube: vis is three-dimensional, [B][T][F] for
    order "btf" and [T][B][F] for "tbf"; model_vis and weights have its shape or are None.  -> those and vis' shape"""
    if order not in ("btf", "tbf"):
        raise ValueError(f'order must be "btf" or "tbf", not {order!r}')
    if be is HOST:
        vis = np.asarray(vis)
    shape = tuple(int(v) for v in vis.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"vis must be a cube of three non-empty axes, not of shape {shape}")
    n = shape[0] * shape[1] * shape[2]

    def flat(x, dt, what):
        if x is None:
            return None
        if be is HOST:
            x = np.asarray(x)
        if tuple(x.shape) != shape:
            raise ValueError(f"{what} must have the shape of vis, {shape}, not {tuple(x.shape)}")
        return stream_array(be, x.reshape(n), dt, n, what)
    (B, T), F = (shape[:2] if order == "btf" else shape[1::-1]), shape[2]
    return (B, T, F, 0 if order == "btf" else 1, flat(vis, be.c128, "vis"), flat(model_vis, be.c128, "model_vis"),
            flat(weights, be.f64, "weights")), shape


def sumthreshold_scalars(levels, nsigma, rho, nlevels, eta, min_count, niter):
    """K, levels, eta_f, eta_t, min_count, niter as gridhip_sumthreshold takes them; levels None: the ladder
    nsigma / rho^k, k = 0 .. nlevels - 1.  levels is a host array of float64 in both forms and goes by address."""
    import math
    if levels is None:
        nsigma, rho, nlevels = float(nsigma), float(rho), int(nlevels)
        if not (math.isfinite(nsigma) and nsigma > 0.0 and math.isfinite(rho) and rho > 0.0):
            raise ValueError("nsigma and rho must be finite and > 0")
        if not 1 <= nlevels <= ST_MAX_STAGES:
            raise ValueError(f"nlevels must be in 1 .. {ST_MAX_STAGES}")
        levels = [nsigma / rho ** k for k in range(nlevels)]
    levels = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).reshape(-1))
    if not 1 <= len(levels) <= ST_MAX_STAGES:
        raise ValueError(f"levels must hold 1 .. {ST_MAX_STAGES} thresholds (windows 1, 2, 4, ...)")
    if not (np.isfinite(levels).all() and (levels > 0.0).all()):
        raise ValueError("every level must be finite and > 0")
    eta_f, eta_t = (float(e) for e in eta)
    if not (0.0 <= eta_f < 1.0 and 0.0 <= eta_t < 1.0):
        raise ValueError("eta must be a pair (eta_f, eta_t) in [0, 1)")
    min_count, niter = int(min_count), int(niter)
    if min_count < 1 or not 0 <= niter <= ST_MAX_ROUNDS:
        raise ValueError(f"min_count must be >= 1 and niter in 0 .. {ST_MAX_ROUNDS}")
    return len(levels), levels, eta_f, eta_t, min_count, niter


RM_MAX_CHANNELS, RM_MAX_DEPTHS, RM_HEAD, RM_MAPS = 1024, 512, 16, 7  # GRIDHIP_RM_* of include/gridhip.h


def rm_table_doubles(C, J):
    """GRIDHIP_RM_TABLE_DOUBLES(C, J): head, E[C][J] complex, R[2J - 1] complex, G[2J - 1]"""
    return RM_HEAD + 2 * C * J + 3 * (2 * J - 1)


def rm_table_args(be, lam2, phi, weights, fwhm):
    """C, J, lam2, weights, phi0, dphi, fwhm as gridhip_rm_tables takes them: lam2 and weights are one-dimensional arrays
    of `be`'s own kind (weights None: all ones), phi = (phi0, dphi, J).  fwhm None: 2 sqrt(3) / (max lam2 - min lam2),
    which for a cuda lam2 is read back (one synchronisation: the table is made once)."""
    import math
    if lam2 is None or (be is not backend(lam2) and be is not HOST):
        raise ValueError(f"lam2 must be a {be.array}")
    lam2 = stream_array(be, lam2, be.f64, -1, "lam2")
    C_ = int(lam2.shape[0])
    weights = stream_array(be, weights, be.f64, C_, "weights")
    try:
        phi0, dphi, J = phi
        phi0, dphi, J = float(phi0), float(dphi), int(J)
    except (TypeError, ValueError):
        raise ValueError("phi must be (phi0, dphi, J)") from None
    if not 1 <= C_ <= RM_MAX_CHANNELS:
        raise ValueError(f"lam2 must hold 1 .. {RM_MAX_CHANNELS} channels, not {C_}")
    if not 1 <= J <= RM_MAX_DEPTHS:
        raise ValueError(f"J must be in 1 .. {RM_MAX_DEPTHS}, not {J}")
    if not (math.isfinite(phi0) and math.isfinite(dphi) and dphi > 0.0):
        raise ValueError("phi0 and dphi must be finite and dphi > 0")
    if fwhm is None:
        span = float(lam2.max() - lam2.min())
        if not (math.isfinite(span) and span > 0.0):
            raise ValueError("fwhm=None needs two different finite lam2 (pass fwhm)")
        fwhm = 2.0 * math.sqrt(3.0) / span
    fwhm = float(fwhm)
    if not (math.isfinite(fwhm) and fwhm > 0.0):
        raise ValueError("fwhm must be finite and > 0")
    return C_, J, lam2, weights, phi0, dphi, fwhm


def rm_table_of(be, tables, C_=None, J=None):
    """tables, C, J: a table of gridhip_rm_tables as the other two entry points take it - one-dimensional float64 of `be`'s
    own kind, in the ABI's form - and its shape, from its length and the one of C and J that the caller's arrays fix."""
    if tables is None or be is not backend(tables) or not be.ok(tables, be.f64) or len(tables.shape) != 1:
        raise ValueError(f"tables must be a one-dimensional float64 {be.array} (Context.rm_tables)")
    n = int(tables.shape[0]) - (RM_HEAD - 3)
    if C_ is not None:
        J = n // (2 * C_ + 6)
    else:
        C_ = (n // J - 6) // 2
    if not (1 <= C_ <= RM_MAX_CHANNELS and 1 <= J <= RM_MAX_DEPTHS and rm_table_doubles(C_, J) == int(tables.shape[0])):
        raise ValueError(f"tables of {int(tables.shape[0])} values do not belong to these arrays")
    return tables, C_, J


def rm_images(be, q, u):
    """M, C, q, u, the shape of a LOS block: q and u are [C, ...] real arrays of one shape, converted where they must be"""
    if q is None or u is None or be is not backend(u) or not hasattr(q, "shape") or not hasattr(u, "shape"):
        raise ValueError(f"q and u must be {be.array}s of one kind")
    shape = tuple(int(v) for v in q.shape)
    if len(shape) < 2 or min(shape) < 1 or tuple(int(v) for v in u.shape) != shape:
        raise ValueError(f"q and u must be of one shape [C, ...] with at least one line of sight, not {shape} and {tuple(u.shape)}")
    for x in (q, u):
        if (x.dtype.kind == "c") if be is HOST else x.dtype.is_complex:
            raise ValueError("q and u must be real")
    if not 1 <= shape[0] <= RM_MAX_CHANNELS:
        raise ValueError(f"q and u must hold 1 .. {RM_MAX_CHANNELS} channels, not {shape[0]}")
    M = 1
    for v in shape[1:]:
        M *= v
    return M, shape[0], be.cv(q, be.f64), be.cv(u, be.f64), shape[1:]


def rm_cube(be, cube):
    """M, J, the shape of a LOS block: the [J, ...] complex128 cube RM-CLEAN updates in place, in the ABI's form"""
    shape = tuple(int(v) for v in getattr(cube, "shape", ()))
    if not (hasattr(cube, "dtype") and be.ok(cube, be.c128)) or len(shape) < 2 or min(shape) < 1:
        raise ValueError(f"cube must be {be.form} of shape [J, ...] (it is updated in place)")
    if not 1 <= shape[0] <= RM_MAX_DEPTHS:
        raise ValueError(f"cube must hold 1 .. {RM_MAX_DEPTHS} depths, not {shape[0]}")
    M = 1
    for v in shape[1:]:
        M *= v
    return M, shape[0], shape[1:]


def rm_clean_scalars(be, gain, threshold, niter, nsigma, noise, restore, like):
    """gain, threshold, niter, nsigma, noise, restore as gridhip_rmclean takes them.  noise: sigma as a number, or one
    float64 element of `be`'s own kind; a NUMBER with device arrays is uploaded by this call and cannot be captured."""
    import math
    gain, threshold, niter, nsigma = float(gain), float(threshold), int(niter), float(nsigma)
    if not (math.isfinite(gain) and math.isfinite(threshold)):
        raise ValueError("gain and threshold must be finite")
    if niter < 0:
        raise ValueError("niter must be >= 0")
    if not (math.isfinite(nsigma) and nsigma >= 0.0):
        raise ValueError("nsigma must be finite and >= 0")
    if noise is None:
        if nsigma > 0.0:
            raise ValueError("nsigma > 0 needs noise (sigma: a number or one float64 element)")
    elif isinstance(noise, (int, float)):
        noise = np.array([noise], dtype=np.float64)
        if be is not HOST:
            noise = be.torch.from_numpy(noise).to(getattr(like, "device", like))
    elif be is not backend(noise) or not be.ok(noise, be.f64) or int(np.prod(tuple(noise.shape))) != 1:
        raise ValueError(f"noise must be a number or a {be.array} of one float64 element")
    return gain, threshold, niter, nsigma, noise, int(bool(restore))


FRINGE_HEAD, FRINGE_PEAK = 16, 12  # GRIDHIP_FRINGE_* of include/gridhip.h
FRINGE_MAX_CHANNELS, FRINGE_MAX_DELAYS, FRINGE_MAX_TINT, FRINGE_MAX_RATES = 1024, 4096, 256, 1024


def fringe_table_doubles(F, T, Nd, Nr):
    """GRIDHIP_FRINGE_TABLE_DOUBLES(F, T, Nd, Nr): head, Ef[F][Nd] and Et[T][Nr] complex, tref[T], a[F], dt[T]"""
    return FRINGE_HEAD + 2 * F * Nd + 2 * T * Nr + 2 * T + F


def fringe_intervals(T, tint):
    """tint after the 0 -> T rule, and I = ceil(T / tint)"""
    tint = int(tint)
    tint = T if tint == 0 else tint
    if not 1 <= tint <= FRINGE_MAX_TINT:
        raise ValueError(f"tint must be in 1 .. {FRINGE_MAX_TINT} (0: all {T} time steps), not {tint}")
    return tint, (T + tint - 1) // tint


def fringe_axis(axis, most, what):
    """(x0, dx, N) of a search axis"""
    import math
    try:
        x0, dx, N = axis
        x0, dx, N = float(x0), float(dx), int(N)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be (first, step, count)") from None
    if not 1 <= N <= most:
        raise ValueError(f"{what} must hold 1 .. {most} cells, not {N}")
    if not (math.isfinite(x0) and math.isfinite(dx) and dx > 0.0):
        raise ValueError(f"{what} must start at a finite value with a finite step > 0")
    return x0, dx, N


def fringe_table_args(be, freq, time, tint, delays, rates):
    """F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr as gridhip_fringe_tables takes them"""
    if freq is None or time is None or be is not backend(time):
        raise ValueError(f"freq and time must be {be.array}s of one kind")
    freq, time = stream_array(be, freq, be.f64, -1, "freq"), stream_array(be, time, be.f64, -1, "time")
    F, T = int(freq.shape[0]), int(time.shape[0])
    if not 1 <= F <= FRINGE_MAX_CHANNELS or T < 1:
        raise ValueError(f"freq must hold 1 .. {FRINGE_MAX_CHANNELS} channels and time at least one step")
    tint, _ = fringe_intervals(T, tint)
    return (F, T, tint, freq, time, *fringe_axis(delays, FRINGE_MAX_DELAYS, "delays"),
            *fringe_axis(rates, FRINGE_MAX_RATES, "rates"))


def fringe_cube(be, vis, model_vis, weights, a1, a2, nant):
    """B, T, F, A, vis, model_vis, wt, a1, a2: the [B, T, F] cube of a fringe call and its antenna pairs"""
    if vis is None or not hasattr(vis, "shape") or len(vis.shape) != 3 or min(int(v) for v in vis.shape) < 1:
        raise ValueError("vis must be a [B, T, F] cube (gridhip.waterfall_layout, order \"btf\")")
    shape = tuple(int(v) for v in vis.shape)
    B, T, F = shape
    A = int(nant)
    if A < 2 or not 1 <= F <= FRINGE_MAX_CHANNELS:
        raise ValueError(f"nant must be >= 2 and the cube must hold 1 .. {FRINGE_MAX_CHANNELS} channels")
    for x, what in ((model_vis, "model_vis"), (weights, "weights")):
        if x is not None and (be is not backend(x) or tuple(int(v) for v in x.shape) != shape):
            raise ValueError(f"{what} must be a {be.array} of vis' shape {shape}")
    if weights is not None and ((weights.dtype.kind == "c") if be is HOST else weights.dtype.is_complex):
        raise ValueError("weights must be real")
    return (B, T, F, A, be.cv(vis, be.c128), be.cv(model_vis, be.c128), be.cv(weights, be.f64),
            _integers(be, a1, B, "a1"), _integers(be, a2, B, "a2"))


def fringe_table_of(be, tables, F, T, tint):
    """tables, I of a table that belongs to a cube of T time steps and F channels: tint is what Context.fringe_tables was
    given, and I = ceil(T / tint) is what the caller's peaks and sol are sized by.  The library compares I with the table's
    head and refuses another (stats[7] = 1, nothing written); a numpy table's head is compared here as well, so that the
    mistake raises."""
    if tables is None or be is not backend(tables) or not be.ok(tables, be.f64) or len(tables.shape) != 1 or \
            int(tables.shape[0]) < FRINGE_HEAD:
        raise ValueError(f"tables must be a one-dimensional float64 {be.array} (Context.fringe_tables)")
    tint, I = fringe_intervals(T, tint)
    if be is HOST and tables[0] == 1.0 and (tables[1], tables[2]) == (F, T) and (tables[3], tables[4]) != (tint, I):
        raise ValueError(f"tables were made with tint = {int(tables[3])} ({int(tables[4])} intervals), not {tint} ({I})")
    return tables, I


def fringe_sol(be, sol, I, A, like, what="sol"):
    """a solution [I][A][4] in the ABI's form, or None"""
    if sol is None:
        return None
    if not (be is backend(sol) and be.ok(sol, be.f64) and tuple(int(v) for v in sol.shape) == (I, A, 4)):
        raise ValueError(f"{what} must be a float64 {be.array} of shape ({I}, {A}, 4): tau, r, Re g, Im g")
    return sol


def fringe_solve_scalars(min_count, min_coh2, refant, niter, tol, A):
    """min_count, min_coh2, refant, niter, tol as gridhip_fringe_solve takes them (refant None: -1)"""
    import math
    min_count, min_coh2, niter, tol = float(min_count), float(min_coh2), int(niter), float(tol)
    refant = -1 if refant is None else int(refant)
    if refant >= A:
        raise ValueError(f"refant must be below nant ({A}), or None")
    if not (math.isfinite(min_count) and min_count >= 0.0 and math.isfinite(min_coh2) and min_coh2 >= 0.0):
        raise ValueError("min_count and min_coh2 must be finite and >= 0")
    if not 0 <= niter <= 100000 or not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError("niter must be in 0 .. 100000 and tol finite and >= 0")
    return min_count, min_coh2, refant, niter, tol


TEC_KAPPA = 1.3445365934456e9  # GRIDHIP_TEC_KAPPA: turns Hz per TEC unit
TEC_HEAD, TEC_PEAK, TEC_MAX_CHANNELS, TEC_MAX_DELAYS, TEC_MAX_CELLS = 16, 12, 1024, 4096, 1024  # GRIDHIP_TEC_*


def tec_table_doubles(F, Nd, Nm):
    """GRIDHIP_TEC_TABLE_DOUBLES(F, Nd, Nm): head, Ef[F][Nd] and Em[F][Nm] complex, a[F], c[F]"""
    return TEC_HEAD + 2 * F * Nd + 2 * F * Nm + 2 * F


def tec_intervals(T, tint):
    """tint after the 0 -> T rule, and I = ceil(T / tint); no cap but T: time is summed before the search"""
    tint = int(tint)
    tint = T if tint == 0 else tint
    if not 1 <= tint <= T:
        raise ValueError(f"tint must be in 1 .. {T} (0: all {T} time steps), not {tint}")
    return tint, (T + tint - 1) // tint


def tec_table_args(be, freq, ntime, tint, delays, tecs):
    """F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm as gridhip_tec_tables takes them"""
    if freq is None:
        raise ValueError(f"freq must be a {be.array}")
    freq = stream_array(be, freq, be.f64, -1, "freq")
    F, T = int(freq.shape[0]), int(ntime)
    if not 1 <= F <= TEC_MAX_CHANNELS or T < 1:
        raise ValueError(f"freq must hold 1 .. {TEC_MAX_CHANNELS} channels and ntime must be at least 1")
    tint, _ = tec_intervals(T, tint)
    return (F, T, tint, freq, *fringe_axis(delays, TEC_MAX_DELAYS, "delays"), *fringe_axis(tecs, TEC_MAX_CELLS, "tecs"))


def tec_table_of(be, tables, F, T, tint):
    """tables, I of a TEC table that belongs to a cube of T time steps and F channels (fringe_table_of's rules)"""
    if tables is None or be is not backend(tables) or not be.ok(tables, be.f64) or len(tables.shape) != 1 or \
            int(tables.shape[0]) < TEC_HEAD:
        raise ValueError(f"tables must be a one-dimensional float64 {be.array} (Context.tec_tables)")
    tint, I = tec_intervals(T, tint)
    if be is HOST and tables[0] == 1.0 and (tables[1], tables[2]) == (F, T) and (tables[3], tables[4]) != (tint, I):
        raise ValueError(f"tables were made with tint = {int(tables[3])} ({int(tables[4])} intervals), not {tint} ({I})")
    return tables, I


CONTSUB_MAX_CHANNELS, CONTSUB_MAX_DEGREE, CONTSUB_ROWINFO, CONTSUB_MAX_ROUNDS = 4096, 3, 4, 4  # GRIDHIP_CONTSUB_*


def contsub_args(be, data, x, mask, weights, degree, axis, mode, nsigma, niter, out, coeffs, info, codes):
    """R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo, codes, stats as
    gridhip_contsub takes them.  data: [..., C] for axis -1 (layout 0) or [C, ...] for axis 0 (layout 1), complex128 (ncomp
    2) or float64 (ncomp 1), in the ABI's form as it is - a cube is never converted or copied; weights (float64) and out
    (data's dtype; it may be data itself) have its shape and form.  x: C real values; mask: C values of dtype bool or uint8,
    or None.  coeffs, info, codes: whether the call makes that output (coeffs [..., D+1] or [D+1, ...] of data's dtype, info
    [..., 4] or [4, ...], codes uint8 of data's shape)."""
    import math
    if axis not in (-1, 0):
        raise ValueError(f"axis must be -1 ([..., C]) or 0 ([C, ...]), not {axis!r}")
    if mode not in ("subtract", "model"):
        raise ValueError(f'mode must be "subtract" or "model", not {mode!r}')
    shape = tuple(int(v) for v in getattr(data, "shape", ()))
    if not hasattr(data, "dtype") or be is not backend(data) or len(shape) < 1 or min(shape) < 1:
        raise ValueError(f"data must be a non-empty {be.array} of dtype complex128 or float64")
    dt = be.c128 if be.ok(data, be.c128) else be.f64
    if not be.ok(data, dt):
        raise ValueError(f"data must be a {be.array} of dtype complex128 or float64, not converted: {data.dtype}")
    C_, rest = (shape[-1], shape[:-1]) if axis == -1 else (shape[0], shape[1:])
    R = 1
    for v in rest:
        R *= v
    degree, niter, nsigma = int(degree), int(niter), float(nsigma)
    if not 1 <= C_ <= CONTSUB_MAX_CHANNELS:
        raise ValueError(f"data must hold 1 .. {CONTSUB_MAX_CHANNELS} channels along axis {axis}, not {C_}")
    if not 0 <= degree <= CONTSUB_MAX_DEGREE or not 0 <= niter <= CONTSUB_MAX_ROUNDS:
        raise ValueError(f"degree must be in 0 .. {CONTSUB_MAX_DEGREE} and niter in 0 .. {CONTSUB_MAX_ROUNDS}")
    if not (math.isfinite(nsigma) and nsigma >= 0.0):
        raise ValueError("nsigma must be finite and >= 0")
    if x is None:
        raise ValueError("x must hold one coordinate per channel (gridhip.channel_coordinate)")
    if be is HOST and (is_torch(x) or is_torch(mask) or is_torch(weights) or is_torch(out)):
        raise ValueError("numpy data takes numpy arguments throughout")
    x = stream_array(be, x, be.f64, C_, "x")
    if be is HOST and mask is not None:
        mask = np.asarray(mask)
    mask = mask_of(be, mask, (C_,))
    if weights is not None and not (be is backend(weights) and be.ok(weights, be.f64) and tuple(weights.shape) == shape):
        raise ValueError(f"weights must be a float64 {be.array} of data's shape {shape}")
    if out is not None and not (be is backend(out) and be.ok(out, dt) and tuple(out.shape) == shape):
        raise ValueError(f"out must be a {be.array} of data's shape and dtype (it is written in place; it may be data)")
    if out is None:
        out = be.empty(shape, dt, data)
    u8 = np.uint8 if be is HOST else be.torch.uint8
    lead = (lambda k: rest + (k,)) if axis == -1 else (lambda k: (k,) + rest)
    coeffs = be.empty(lead(degree + 1), dt, data) if coeffs else None
    info = be.empty(lead(CONTSUB_ROWINFO), be.f64, data) if info else None
    codes = be.empty(shape, u8, data) if codes else None
    stats = be.empty(8, be.f64, data)
    return (R, C_, 0 if axis == -1 else 1, 2 if dt is be.c128 else 1, degree, 0 if mode == "subtract" else 1, x, mask, data,
            weights, nsigma, niter, out, coeffs, info, codes, stats)


COMP_DOUBLES = 10  # GRIDHIP_COMP_DOUBLES: { l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0 }


def component_list(be, comps):
    """C, comps as gridhip_dft_predict takes a component list: a (C, 10) float64 array of `be`'s own kind (the rows of
    gridhip.components or of Context.components_from_image), converted where it must be"""
    if be is not backend(comps) or not hasattr(comps, "shape"):
        raise ValueError(f"comps must be a {be.array} of shape (C, {COMP_DOUBLES})")
    if len(comps.shape) != 2 or int(comps.shape[1]) != COMP_DOUBLES:
        raise ValueError(f"comps must be of shape (C, {COMP_DOUBLES}), not {tuple(comps.shape)}")
    if comps.dtype.kind == "c" if be is HOST else comps.dtype.is_complex:
        raise ValueError(f"comps must be real, not {comps.dtype}")
    return int(comps.shape[0]), be.cv(comps, be.f64)


def component_count(be, count, like):
    """count as gridhip_dft_predict takes it, or None: one int64 element of `be`'s own kind - on the device nothing is read
    back - or, for host arrays, a number"""
    if count is None:
        return None
    if be is HOST and isinstance(count, (int, np.integer)):
        return np.array([count], dtype=np.int64)
    if be is not backend(count) or not be.ok(count, be.i64) or int(np.prod(tuple(count.shape))) != 1:
        raise ValueError(f"count must be a {be.array} of one int64 element" + (" or an int" if be is HOST else ""))
    return count


def group_ids(be, group, G, n):
    """G, group as gridhip_average takes them: group None goes as NULL and needs G in (None, 1); a given group needs G, the
    number of groups (gridhip.average_groups and gridhip.flag_groups return both)"""
    if group is None:
        if G not in (None, 1):
            raise ValueError("G > 1 needs group, the group of every visibility")
        return 1, None
    if G is None:
        raise ValueError("group needs G, the number of groups (average_groups returns both)")
    if int(G) < 1:
        raise ValueError("G must be >= 1")
    return int(G), _integers(be, group, n, "group")


def rotation(R):
    """R as gridhip_phase_shift and gridhip_average take it: 9 host float64 values whichever back end the stream comes from,
    passed by address - the caller keeps the returned array alive for the call; None goes as NULL.  The values are checked by
    the library (finite, R22 > 0, orthonormal to 1e-9)."""
    if R is None:
        return None, None
    if is_torch(R):
        R = R.detach().cpu().numpy()
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.shape not in ((3, 3), (9,)):
        raise ValueError(f"R must be a 3 x 3 rotation, not of shape {R.shape}")
    return R.ctypes.data_as(C.POINTER(C.c_double)), R


MOSAIC_KINDS = {"nearest": 0, "bilinear": 1, "cubic": 3}  # gridhip_mosaic's kind


def facet_rotations(be, R, F, like):
    """R as gridhip_mosaic takes it: (F, 9) float64 of `be`'s own kind.  A host array - (F, 3, 3), (F, 9), or one 3 x 3
    rotation when F == 1 - is checked here by the library's rule (finite, R22 > 0, orthonormal to 1e-9) and, for cuda
    facets, uploaded; a cuda tensor is left to the rule on the device, where a bad facet is counted and left out."""
    if is_torch(R) and R.is_cuda:
        if be is HOST:
            raise ValueError("R must be a host array when the facets are numpy arrays")
        R = be.cv(R, be.f64)
        if R.numel() != 9 * F:
            raise ValueError(f"R must hold one 3 x 3 rotation per facet ({F}), not {tuple(R.shape)}")
        return R.reshape(F, 9)
    if is_torch(R):
        R = R.detach().numpy()
    R = np.ascontiguousarray(R, dtype=np.float64)
    if R.size != 9 * F or R.shape[-1] not in (3, 9):
        raise ValueError(f"R must hold one 3 x 3 rotation per facet ({F}), not {R.shape}")
    R = R.reshape(F, 9)
    M = R.reshape(F, 3, 3)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(R).all(axis=1) | ~(R[:, 8] > 0.0)
        bad |= ~(np.abs(M @ M.transpose(0, 2, 1) - np.eye(3)) <= 1e-9).all(axis=(1, 2))
    if bad.any():
        raise ValueError(f"R of facet {int(np.flatnonzero(bad)[0])} is not a rotation with R22 > 0 (finite, |R R^T - I| <= 1e-9)")
    return R if be is HOST else be.torch.from_numpy(R).to(getattr(like, "device", like))


def mosaic_args(be, facets, theta_src, R, theta_dst, N_dst, kind, weights, window, normalize, wmin, blank, wsum, stats, out):
    """F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out, wsum, stats as
    gridhip_mosaic[_dev] takes them (include/gridhip.h, "reprojection and mosaicking").  facets: (F, Ns, Ns) or one
    (Ns, Ns) image; window: (inner, outer) in facet cells, None for inner = outer = Ns / 2."""
    import math
    given = shape = tuple(getattr(facets, "shape", ()))
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1] != shape[2] or min(shape) < 1:
        raise ValueError(f"facets must be (F, Ns, Ns) square images, not {shape}")
    F, Ns, Nd = shape[0], shape[1], int(N_dst)
    if Nd < 1:
        raise ValueError("N_dst must be >= 1")
    if be is HOST:
        facets = np.asarray(facets)
    if (facets.dtype.kind == "c") if be is HOST else facets.dtype.is_complex:
        raise ValueError(f"facets must be real, not {facets.dtype}")
    facets = be.cv(facets, be.f64)
    if weights is not None:
        if be is not backend(weights) or tuple(weights.shape) != given:
            raise ValueError(f"weights must be a {be.array} of the facets' shape {given}, or None")
        weights = be.cv(weights, be.f64)
    if kind not in MOSAIC_KINDS:
        raise ValueError(f"kind must be one of {sorted(MOSAIC_KINDS)}, not {kind!r}")
    theta_s, theta_d = float(theta_src), float(theta_dst)
    if not (math.isfinite(theta_s) and theta_s > 0.0 and math.isfinite(theta_d) and theta_d > 0.0):
        raise ValueError("theta_src and theta_dst must be finite and > 0")
    inner, outer = (Ns / 2, Ns / 2) if window is None else (float(window[0]), float(window[1]))
    if not (math.isfinite(inner) and math.isfinite(outer) and 0.0 <= inner <= outer):
        raise ValueError("window must be (inner, outer) in cells with 0 <= inner <= outer")
    wmin = float(wmin)
    if not wmin >= 0.0:
        raise ValueError("wmin must be >= 0")
    R = facet_rotations(be, R, F, facets)
    out = result_array(be, out, be.f64, (Nd, Nd), "out", facets)
    ws = be.empty((Nd, Nd), be.f64, facets) if wsum else None
    st8 = be.empty(8, be.f64, facets) if stats else None
    return (F, Ns, theta_s, facets, weights, R, MOSAIC_KINDS[kind], inner, outer, int(bool(normalize)), wmin, float(blank), Nd,
            theta_d, out, ws, st8)


SRC_DOUBLES = 16  # GRIDHIP_SRC_DOUBLES: { label, ncells, yp, xp, peak, S, Sx, Sy, Sxx, Sxy, Syy, y0, y1, x0, x1, flags }


def source_args(be, thr, nsigma, noise, peak_frac, min_cells, beam, correct, max_sources, out, info, like):
    """thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam, correct, max_c, comps, info, count, stats as
    the find_sources entry points take them (include/gridhip.h, "source finding"): the levels as for automask_args; beam:
    the 8 values of fit_beam as an array of `be`'s own kind, or None; out: the (max_sources, 10) array to write, or None
    for a new one of zeros; info: whether the (max_sources, 16) table of measurements is wanted."""
    levels = automask_args(be, False, thr, nsigma, noise, peak_frac, min_cells, 0, like)[1:8]
    max_c = int(max_sources)
    if max_c < 0:
        raise ValueError("max_sources must be >= 0")
    if beam is not None:
        if be is not backend(beam) or not hasattr(beam, "shape") or tuple(beam.shape) != (8,):
            raise ValueError(f"beam must be the 8 values of fit_beam as a {be.array}, or None")
        beam = be.cv(beam, be.f64)
    if out is None:
        out = be.zeros((max_c, COMP_DOUBLES), be.f64, like)
    else:
        out = result_array(be, out, be.f64, (max_c, COMP_DOUBLES), "out", like)
    table = be.zeros((max_c, SRC_DOUBLES), be.f64, like) if info else None
    return (*levels, beam, int(bool(correct)), max_c, out, table, be.zeros(1, be.i64, like), be.empty(8, be.f64, like))


def model_planes(be, model, N):
    """T, model as gridhip_components_from_image takes a model: (N, N), or (T, N, N) with T in 1..4, float64"""
    shape = tuple(getattr(model, "shape", ()))
    if shape == (N, N):
        shape = (1, N, N)
    if len(shape) != 3 or shape[1:] != (N, N) or not 1 <= shape[0] <= 4:
        raise ValueError(f"model must be {N} x {N} (image_size(theta, lam)) or T of them, T in 1..4, not {shape}")
    return shape[0], be.cv(model, be.f64)


class Handle:
    """Owner of one library handle `_h` (a context, plan, imager or communicator): destroyed once, by close() or by the
    collector; _call passes it to an entry point and raises GridHipError with the owner's last-error text."""
    _destroy = _what = None  # gridhip_*_destroy; the name _open() refuses by
    _ctx = None              # the Context whose stream a device call runs on

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        assert self._h, f"{self._what} is closed"

    def _check(self, rc):
        if rc != 0:
            raise GridHipError(rc, self._error(rc))

    def _call(self, be, name, *args):
        """gridhip_<name>(handle, args...) for host arguments, gridhip_<name>_dev on torch's current stream for device
        arguments.  The arguments the prototype takes as `void *` are arrays (or None) and go by address, everything
        else as it is."""
        be.bind(self)
        name = "gridhip_" + name + be.suffix
        args, ptr = list(args), be.ptr
        for i in POINTERS[name]:
            if args[i] is not None:
                args[i] = ptr(args[i])
        self._check(getattr(self._lib, name)(self._h, *args))
