"""ctypes loader for libgridhip.so (the C ABI declared in include/gridhip.h).

There is no CPU fallback: if the HIP library has not been built this module raises, and every
compute entry point needs a gfx950 device.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(_PKG, "..", ".."))          # ska-sdp-accelerate-gridding_amd/
# GRIDHIP_LIB: another build of the same ABI (tools/ use lib/libgridhip_tuning.so, which has the "dbg" option)
LIB_PATH = os.environ.get("GRIDHIP_LIB") or os.path.join(ROOT, "lib", "libgridhip.so")

i64 = C.c_int64
vp = C.c_void_p
ci = C.c_int

OK = 0
EINVAL, ENOMEM, EHIP, ENODEV, EUNSUPPORTED = -1, -2, -3, -4, -5

# name -> (restype, argtypes); mirrors include/gridhip.h one to one (tests/test_abi.py compares the two); a host form and
# its _dev twin share one list
_GRID_DEV = [vp, i64, i64, vp, i64, vp, vp, i64, vp]
_CONV_DEV = [vp, i64, i64, vp, i64, i64, i64, i64, vp, vp, vp, i64, vp]
_CONV2_DEV = [vp, i64, i64, vp, i64, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp]
_W_CACHE = [vp, i64, i64, i64, i64, C.c_double, i64, i64, vp, vp, vp, i64, vp, vp]
_AWGRID = [vp, i64, i64, vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp]
_AW_IMAGING = [vp, C.c_double, i64, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp]
_DO_IMAGING = [vp, ci, i64, i64, i64, i64, i64, vp, C.c_double, i64, i64, vp, vp, vp, i64, vp, vp, vp,
               C.POINTER(C.c_double)]
_DO_IMAGING_AW = [vp, C.c_double, i64, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp,
           C.POINTER(C.c_double)]
_AW_GRIDDING = [vp, C.c_double, i64, C.c_double, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp,
                C.POINTER(C.c_double)]
_PREDICT = [vp, ci, i64, i64, i64, i64, i64, vp, C.c_double, i64, vp, i64, vp, vp, vp, i64, vp, vp]
_CLEAN = [vp, i64, vp, vp, vp, C.c_double, C.c_double, i64, i64, i64, vp]
_MFCLEAN = [vp, i64, i64, vp, vp, vp, C.c_double, C.c_double, i64, i64, i64, vp]
_HOST_F64 = C.POINTER(C.c_double)  # an array that is the host's in every form (msclean's scales and bias)
_MSCLEAN = [vp, i64, vp, vp, vp, i64, _HOST_F64, _HOST_F64, C.c_double, C.c_double, i64, i64, i64, vp]
_AUTO = [vp, C.c_double, vp, C.c_double]  # mask, nsigma, noise, peak_frac (the _auto forms, before stats)
_CLEAN_AUTO = _CLEAN[:-1] + _AUTO + [vp]
_MSCLEAN_AUTO = _MSCLEAN[:-1] + _AUTO + [vp]
# N, P, Q, psfs, residuals, models, weights (the host's in both forms), metric, then clean's scalars, _AUTO and stats
_JCLEAN = [vp, i64, i64, i64, vp, vp, vp, _HOST_F64, ci, C.c_double, C.c_double, i64, i64, i64, *_AUTO, vp]
_IMAGE_STATS = [vp, i64, vp, vp, i64, vp]
# border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, grow (automask, after image and mask)
_AUTOMASK_ARGS = [i64, ci, C.c_double, C.c_double, C.c_double, C.c_double, vp, C.c_double, i64, i64]
_AUTOMASK = [vp, i64, vp, vp, *_AUTOMASK_ARGS, vp]
# what the _automask deconvolves take after patch: mask, nsigma, peak_frac_clean, then automask's own from absolute on
# (no border, no noise), then stats, istats, astats
_AUTOMASK_LOOP = [vp, C.c_double, C.c_double, ci, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, i64, i64,
                  vp, vp, vp]
# N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, nodes, background, rms, out, stats
_NOISE_MAP = [vp, i64, vp, vp, ci, i64, i64, i64, C.c_double, i64, i64, ci, vp, vp, vp, vp, vp]
_FIT_BEAM = [vp, i64, vp, i64, C.c_double, vp]
_RESTORE = [vp, i64, vp, vp, vp, i64, vp]
_WEIGHTS = [vp, C.c_double, i64, i64, vp, vp, i64, vp, ci, C.c_double, C.c_double, vp, vp]
_WEIGHTING = [ci, C.c_double, C.c_double, vp]  # mode, robust, taper_sigma, wt_in
_GAINCAL = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, ci, i64, ci, i64, C.c_double, vp, vp]
_APPLY_GAINS = [vp, i64, i64, i64, vp, vp, vp, vp, ci, vp, vp, vp, vp]
_DDCAL = [vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, ci, i64, ci, i64, C.c_double, vp, vp]  # gaincal's, D after T
_STOKES = [vp, i64, ci, ci, ci, vp, vp]  # n, basis, which, inverse, vis, stokes
_DD_SUBTRACT = [vp, i64, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp, vp]
_FLAG_ARGS = [C.c_double, C.c_double, i64, i64, vp, vp, vp, vp]  # nsigma, amax, min_count, niter, then the four outputs
_FLAG = [vp, i64, i64, vp, vp, vp, vp, *_FLAG_ARGS]
# ctx, B, T, F, order, vis, model_vis, wt_in, K, levels (a host array in both forms), eta_f, eta_t, min_count, niter, outputs
_SUMTHRESHOLD = [vp, i64, i64, i64, ci, vp, vp, vp, i64, C.POINTER(C.c_double), C.c_double, C.c_double, i64, i64, vp, vp, vp, vp]
# every array is of the form's own kind (lam2, weights and noise too): C, J, lam2, weights, phi0, dphi, fwhm, tables
_RM_TABLES = [vp, i64, i64, vp, vp, C.c_double, C.c_double, C.c_double, vp]
_RMSYNTH = [vp, i64, i64, i64, vp, vp, vp, vp, vp]  # M, C, J, tables, Q, U, cube, stats
# M, J, tables, cube, model, gain, threshold, niter, nsigma, noise, restore, maps, stats
_RMCLEAN = [vp, i64, i64, vp, vp, vp, C.c_double, C.c_double, i64, C.c_double, vp, ci, vp, vp]
# ctx, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo, codes, stats
_CONTSUB = [vp, i64, i64, ci, ci, ci, ci, vp, vp, vp, vp, C.c_double, i64, vp, vp, vp, vp, vp]
# F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables
_FRINGE_TABLES = [vp, i64, i64, i64, vp, vp, C.c_double, C.c_double, i64, C.c_double, C.c_double, i64, vp]
# B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats
_FRINGE_SEARCH = [vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp]
# B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info, stats
_FRINGE_SOLVE = [vp, i64, i64, i64, vp, vp, vp, C.c_double, C.c_double, i64, i64, C.c_double, vp, vp, vp]
# B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, then the solve's scalars, warm, sol, peaks, info, stats
_FRINGEFIT = [vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp, i64, i64, i64, C.c_double, C.c_double, i64, i64,
              C.c_double, ci, vp, vp, vp, vp]
# B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out
_APPLY_FRINGE = [vp, i64, i64, i64, i64, i64, vp, vp, vp, vp, ci, vp, vp, vp, vp]
# F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables (the search, the driver and the apply step: the fringe lists)
_TEC_TABLES = [vp, i64, i64, i64, vp, C.c_double, C.c_double, i64, C.c_double, C.c_double, i64, vp]
_DFT_PREDICT = [vp, i64, vp, vp, ci, i64, vp, vp, vp, i64, vp, vp, vp, vp]
_COMPONENTS = [vp, C.c_double, i64, ci, vp, i64, vp, vp]
# border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam, correct, max_c, comps, info, count, stats
# (find_sources, after the image)
_FIND_SOURCES_ARGS = [i64, C.c_double, C.c_double, C.c_double, C.c_double, vp, C.c_double, i64, vp, ci, i64, vp, vp, vp, vp]
_FIND_SOURCES = [vp, C.c_double, i64, vp, *_FIND_SOURCES_ARGS]
# R is the host's in both forms (9 doubles, read at the call)
_PHASE_SHIFT = [vp, i64, _HOST_F64, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]
_AVERAGE = [vp, i64, i64, vp, _HOST_F64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
# F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out, wsum, stats; R is an
# array of the form's own kind (host memory in the host form, device memory in the _dev form)
_MOSAIC = [vp, i64, i64, C.c_double, vp, vp, vp, ci, C.c_double, C.c_double, ci, C.c_double, C.c_double, i64, C.c_double,
           vp, vp, vp]
_REPROJECT = [vp, i64, C.c_double, vp, vp, ci, C.c_double, C.c_double, C.c_double, i64, C.c_double, vp]
# wstep, M, qpx, npixFF, npixKern, theta, lam (the stack's shape), then the stream n, u, v, w, uv_stride
_WSTACK = [vp, i64, i64, i64, i64, i64, C.c_double, i64]
_WSTACK_STREAM = [i64, vp, vp, vp, i64]
_PREDICT_AW = [vp, C.c_double, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp]
SIGNATURES = {
    "gridhip_version": (ci, []),
    "gridhip_strerror": (C.c_char_p, [ci]),
    "gridhip_device_count": (ci, [C.POINTER(ci)]),
    "gridhip_create": (ci, [ci, C.POINTER(vp)]),
    "gridhip_destroy": (ci, [vp]),
    "gridhip_last_error": (C.c_char_p, [vp]),
    "gridhip_set_stream": (ci, [vp, vp]),
    "gridhip_reset_stream": (ci, [vp]),
    "gridhip_get_stream": (vp, [vp]),
    "gridhip_synchronize": (ci, [vp]),
    "gridhip_set_option": (ci, [vp, C.c_char_p, i64]),
    "gridhip_get_option": (ci, [vp, C.c_char_p, C.POINTER(i64)]),
    "gridhip_last_dropped": (ci, [vp, C.POINTER(i64)]),
    "gridhip_grid": (ci, _GRID_DEV),
    "gridhip_convgrid": (ci, _CONV_DEV),
    "gridhip_convgrid2": (ci, _CONV2_DEV),
    "gridhip_degrid2": (ci, _CONV2_DEV),
    "gridhip_grid_dev": (ci, _GRID_DEV),
    "gridhip_convgrid_dev": (ci, _CONV_DEV),
    "gridhip_convgrid2_dev": (ci, _CONV2_DEV),
    "gridhip_degrid2_dev": (ci, _CONV2_DEV),
    "gridhip_plan_create_dev": (ci, [vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, i64, vp, C.POINTER(vp)]),
    "gridhip_plan_grid_dev": (ci, [vp, vp, vp, vp]),
    "gridhip_plan_degrid_dev": (ci, [vp, vp, vp, vp]),
    "gridhip_plan_destroy": (ci, [vp]),
    "gridhip_image_size": (i64, [C.c_double, i64]),
    "gridhip_wbins": (ci, [vp, i64, vp, i64, vp, C.POINTER(i64), C.POINTER(i64)]),
    "gridhip_find_closest": (ci, [vp, i64, vp, i64, vp, vp]),
    "gridhip_mirror_uvw": (ci, [vp, i64, vp, vp, vp, vp]),
    "gridhip_doweight": (ci, [vp, C.c_double, i64, i64, vp, vp, vp]),
    "gridhip_make_grid_hermitian": (ci, [vp, i64, vp]),
    "gridhip_fft2_centered": (ci, [vp, i64, vp, vp, ci]),
    "gridhip_w_kernel": (ci, [vp, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_simple_imaging": (ci, [vp, C.c_double, i64, i64, vp, vp, i64, vp, vp]),
    "gridhip_conv_imaging": (ci, [vp, i64, i64, i64, vp, C.c_double, i64, i64, vp, vp, i64, vp, vp]),
    "gridhip_w_cache_imaging": (ci, _W_CACHE),
    "gridhip_awgrid": (ci, _AWGRID),
    "gridhip_awgrid_dev": (ci, _AWGRID),
    "gridhip_aw_last_stats": (ci, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "gridhip_awdegrid": (ci, _AWGRID),
    "gridhip_awdegrid_dev": (ci, _AWGRID),
    "gridhip_aw_plan_create_dev": (ci, [vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, i64, vp, vp, vp,
                                        C.POINTER(vp)]),
    "gridhip_aw_plan_grid_dev": (ci, [vp, vp, vp]),
    "gridhip_aw_plan_degrid_dev": (ci, [vp, vp, vp]),
    "gridhip_aw_plan_destroy": (ci, [vp]),
    "gridhip_aw_imaging": (ci, _AW_IMAGING),
    "gridhip_aw_imaging_dev": (ci, _AW_IMAGING),
    "gridhip_do_imaging_aw": (ci, _DO_IMAGING_AW),
    "gridhip_do_imaging_aw_dev": (ci, _DO_IMAGING_AW),
    "gridhip_aw_gridding": (ci, _AW_GRIDDING),
    "gridhip_aw_gridding_dev": (ci, _AW_GRIDDING),
    "gridhip_do_imaging": (ci, _DO_IMAGING),
    "gridhip_do_imaging_dev": (ci, _DO_IMAGING),
    "gridhip_w_cache_imaging_dev": (ci, _W_CACHE),
    "gridhip_predict": (ci, _PREDICT),
    "gridhip_predict_dev": (ci, _PREDICT),
    "gridhip_predict_aw": (ci, _PREDICT_AW),
    "gridhip_predict_aw_dev": (ci, _PREDICT_AW),
    "gridhip_imager_create_dev": (ci, [vp, ci, i64, i64, i64, i64, i64, vp, C.c_double, i64, i64, vp, vp, vp, i64,
                                       C.POINTER(vp)]),
    "gridhip_imager_create_aw_dev": (ci, [vp, C.c_double, i64, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, i64, vp,
                                          vp, C.POINTER(vp)]),
    "gridhip_imager_psf_dev": (ci, [vp, vp, C.POINTER(C.c_double)]),
    "gridhip_imager_cycle_dev": (ci, [vp, vp, vp, vp, vp]),
    "gridhip_imager_predict_dev": (ci, [vp, vp, vp, vp]),
    "gridhip_imager_destroy": (ci, [vp]),
    "gridhip_clean": (ci, _CLEAN),
    "gridhip_clean_dev": (ci, _CLEAN),
    "gridhip_imager_clean_dev": (ci, [vp, vp, vp, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_imager_deconvolve_dev": (ci, [vp, vp, vp, vp, i64, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_msclean": (ci, _MSCLEAN),
    "gridhip_msclean_dev": (ci, _MSCLEAN),
    "gridhip_imager_msclean_dev": (ci, [vp, vp, vp, i64, _HOST_F64, _HOST_F64, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_imager_msdeconvolve_dev": (ci, [vp, vp, vp, vp, i64, i64, _HOST_F64, _HOST_F64, C.c_double, C.c_double, i64,
                                             i64, i64, vp]),
    "gridhip_image_stats": (ci, _IMAGE_STATS),
    "gridhip_image_stats_dev": (ci, _IMAGE_STATS),
    "gridhip_imager_image_stats_dev": (ci, [vp, vp, vp, i64, vp]),
    "gridhip_clean_auto": (ci, _CLEAN_AUTO),
    "gridhip_clean_auto_dev": (ci, _CLEAN_AUTO),
    "gridhip_msclean_auto": (ci, _MSCLEAN_AUTO),
    "gridhip_msclean_auto_dev": (ci, _MSCLEAN_AUTO),
    "gridhip_imager_clean_auto_dev": (ci, [vp, vp, vp, C.c_double, C.c_double, i64, i64, i64, *_AUTO, vp]),
    "gridhip_imager_msclean_auto_dev": (ci, [vp, vp, vp, i64, _HOST_F64, _HOST_F64, C.c_double, C.c_double, i64, i64, i64,
                                             *_AUTO, vp]),
    "gridhip_imager_deconvolve_auto_dev": (ci, [vp, vp, vp, vp, i64, C.c_double, C.c_double, i64, i64, i64, vp, C.c_double,
                                                C.c_double, vp, vp]),
    "gridhip_imager_msdeconvolve_auto_dev": (ci, [vp, vp, vp, vp, i64, i64, _HOST_F64, _HOST_F64, C.c_double, C.c_double,
                                                  i64, i64, i64, vp, C.c_double, C.c_double, vp, vp]),
    "gridhip_automask": (ci, _AUTOMASK),
    "gridhip_automask_dev": (ci, _AUTOMASK),
    "gridhip_imager_automask_dev": (ci, [vp, vp, vp, *_AUTOMASK_ARGS, vp]),
    "gridhip_imager_deconvolve_automask_dev": (ci, [vp, vp, vp, vp, i64, C.c_double, C.c_double, i64, i64, i64,
                                                    *_AUTOMASK_LOOP]),
    "gridhip_imager_msdeconvolve_automask_dev": (ci, [vp, vp, vp, vp, i64, i64, _HOST_F64, _HOST_F64, C.c_double,
                                                      C.c_double, i64, i64, i64, *_AUTOMASK_LOOP]),
    "gridhip_noise_map_nodes": (i64, [i64, i64, i64]),
    "gridhip_noise_map": (ci, _NOISE_MAP),
    "gridhip_noise_map_dev": (ci, _NOISE_MAP),
    "gridhip_fit_beam": (ci, _FIT_BEAM),
    "gridhip_fit_beam_dev": (ci, _FIT_BEAM),
    "gridhip_restore": (ci, _RESTORE),
    "gridhip_restore_dev": (ci, _RESTORE),
    "gridhip_imager_beam_dev": (ci, [vp, i64, C.c_double, vp]),
    "gridhip_imager_restore_dev": (ci, [vp, vp, vp, i64, C.c_double, i64, vp, vp]),
    "gridhip_weights": (ci, _WEIGHTS),
    "gridhip_weights_dev": (ci, _WEIGHTS),
    "gridhip_imager_create_weighted_dev": (ci, [vp, ci, i64, i64, i64, i64, i64, vp, C.c_double, i64, i64, vp, vp, vp, i64,
                                                *_WEIGHTING, C.POINTER(vp)]),
    "gridhip_imager_create_aw_weighted_dev": (ci, [vp, C.c_double, i64, i64, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp,
                                                   i64, vp, vp, *_WEIGHTING, C.POINTER(vp)]),
    "gridhip_imager_weight_stats_dev": (ci, [vp, vp]),
    "gridhip_mfclean": (ci, _MFCLEAN),
    "gridhip_mfclean_dev": (ci, _MFCLEAN),
    "gridhip_imager_set_spectral_dev": (ci, [vp, i64, vp]),
    "gridhip_imager_spectral_psfs_dev": (ci, [vp, vp]),
    "gridhip_imager_mfs_cycle_dev": (ci, [vp, vp, vp, vp, vp]),
    "gridhip_imager_mfclean_dev": (ci, [vp, vp, vp, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_imager_mfdeconvolve_dev": (ci, [vp, vp, vp, vp, i64, C.c_double, C.c_double, i64, i64, i64, vp]),
    "gridhip_gaincal": (ci, _GAINCAL),
    "gridhip_gaincal_dev": (ci, _GAINCAL),
    "gridhip_apply_gains": (ci, _APPLY_GAINS),
    "gridhip_apply_gains_dev": (ci, _APPLY_GAINS),
    "gridhip_imager_selfcal_dev": (ci, [vp, vp, vp, i64, i64, vp, vp, vp, vp, ci, i64, ci, i64, C.c_double, vp, vp, vp, vp]),
    "gridhip_ddcal": (ci, _DDCAL),
    "gridhip_ddcal_dev": (ci, _DDCAL),
    "gridhip_ddcal_lds_antennas": (i64, [i64]),
    "gridhip_dd_subtract": (ci, _DD_SUBTRACT),
    "gridhip_dd_subtract_dev": (ci, _DD_SUBTRACT),
    "gridhip_imager_peel_dev": (ci, [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, ci, i64, ci, i64, C.c_double, vp, vp, vp, vp,
                                     vp]),
    "gridhip_jonescal": (ci, _GAINCAL),
    "gridhip_jonescal_dev": (ci, _GAINCAL),
    "gridhip_jonescal_lds_antennas": (i64, []),
    "gridhip_apply_jones": (ci, _APPLY_GAINS),
    "gridhip_apply_jones_dev": (ci, _APPLY_GAINS),
    "gridhip_stokes": (ci, _STOKES),
    "gridhip_stokes_dev": (ci, _STOKES),
    "gridhip_flag_residuals": (ci, _FLAG),
    "gridhip_flag_residuals_dev": (ci, _FLAG),
    "gridhip_imager_flag_dev": (ci, [vp, vp, vp, i64, vp, vp, *_FLAG_ARGS]),
    "gridhip_sumthreshold": (ci, _SUMTHRESHOLD),
    "gridhip_sumthreshold_dev": (ci, _SUMTHRESHOLD),
    "gridhip_sumthreshold_tile": (ci, [C.POINTER(i64), C.POINTER(i64)]),
    "gridhip_rm_tables": (ci, _RM_TABLES),
    "gridhip_rm_tables_dev": (ci, _RM_TABLES),
    "gridhip_rmsynth": (ci, _RMSYNTH),
    "gridhip_rmsynth_dev": (ci, _RMSYNTH),
    "gridhip_rmclean": (ci, _RMCLEAN),
    "gridhip_rmclean_dev": (ci, _RMCLEAN),
    "gridhip_rm_tile": (ci, [C.POINTER(i64)]),
    "gridhip_contsub": (ci, _CONTSUB),
    "gridhip_contsub_dev": (ci, _CONTSUB),
    "gridhip_contsub_tile": (ci, [C.POINTER(i64)]),
    "gridhip_fringe_tables": (ci, _FRINGE_TABLES),
    "gridhip_fringe_tables_dev": (ci, _FRINGE_TABLES),
    "gridhip_fringe_search": (ci, _FRINGE_SEARCH),
    "gridhip_fringe_search_dev": (ci, _FRINGE_SEARCH),
    "gridhip_fringe_solve": (ci, _FRINGE_SOLVE),
    "gridhip_fringe_solve_dev": (ci, _FRINGE_SOLVE),
    "gridhip_fringefit": (ci, _FRINGEFIT),
    "gridhip_fringefit_dev": (ci, _FRINGEFIT),
    "gridhip_apply_fringe": (ci, _APPLY_FRINGE),
    "gridhip_apply_fringe_dev": (ci, _APPLY_FRINGE),
    "gridhip_fringe_tile": (ci, [C.POINTER(i64)]),
    "gridhip_tec_tables": (ci, _TEC_TABLES),
    "gridhip_tec_tables_dev": (ci, _TEC_TABLES),
    "gridhip_tec_search": (ci, _FRINGE_SEARCH),
    "gridhip_tec_search_dev": (ci, _FRINGE_SEARCH),
    "gridhip_tecfit": (ci, _FRINGEFIT),
    "gridhip_tecfit_dev": (ci, _FRINGEFIT),
    "gridhip_apply_tec": (ci, _APPLY_FRINGE),
    "gridhip_apply_tec_dev": (ci, _APPLY_FRINGE),
    "gridhip_tec_tile": (ci, [C.POINTER(i64)]),
    "gridhip_dft_predict": (ci, _DFT_PREDICT),
    "gridhip_dft_predict_dev": (ci, _DFT_PREDICT),
    "gridhip_components_from_image": (ci, _COMPONENTS),
    "gridhip_components_from_image_dev": (ci, _COMPONENTS),
    "gridhip_find_sources": (ci, _FIND_SOURCES),
    "gridhip_find_sources_dev": (ci, _FIND_SOURCES),
    "gridhip_imager_find_sources_dev": (ci, [vp, vp, *_FIND_SOURCES_ARGS]),
    "gridhip_phase_shift": (ci, _PHASE_SHIFT),
    "gridhip_phase_shift_dev": (ci, _PHASE_SHIFT),
    "gridhip_average": (ci, _AVERAGE),
    "gridhip_average_dev": (ci, _AVERAGE),
    "gridhip_mosaic": (ci, _MOSAIC),
    "gridhip_mosaic_dev": (ci, _MOSAIC),
    "gridhip_reproject": (ci, _REPROJECT),
    "gridhip_reproject_dev": (ci, _REPROJECT),
    "gridhip_wstack_create_dev": (ci, _WSTACK + _WSTACK_STREAM + [C.POINTER(vp)]),
    "gridhip_wstack_image_dev": (ci, [vp, vp, vp]),
    "gridhip_wstack_predict_dev": (ci, [vp, vp, vp, vp]),
    "gridhip_wstack_info": (ci, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
    "gridhip_wstack_destroy": (ci, [vp]),
    "gridhip_do_imaging_wstack": (ci, _WSTACK + _WSTACK_STREAM + [vp, vp, vp, C.POINTER(C.c_double)]),
    "gridhip_do_imaging_wstack_dev": (ci, _WSTACK + _WSTACK_STREAM + [vp, vp, vp, C.POINTER(C.c_double)]),
    "gridhip_predict_wstack": (ci, _WSTACK + [vp] + _WSTACK_STREAM + [vp, vp]),
    "gridhip_predict_wstack_dev": (ci, _WSTACK + [vp] + _WSTACK_STREAM + [vp, vp]),
    "gridhip_jclean": (ci, _JCLEAN),
    "gridhip_jclean_dev": (ci, _JCLEAN),
    "gridhip_comm_create": (ci, [ci, C.POINTER(ci), C.POINTER(vp)]),
    "gridhip_comm_unique_id": (ci, [vp]),
    "gridhip_comm_create_rank": (ci, [vp, ci, ci, vp, C.POINTER(vp)]),
    "gridhip_comm_destroy": (ci, [vp]),
    "gridhip_comm_last_error": (C.c_char_p, [vp]),
    "gridhip_comm_ndev": (ci, [vp]),
    "gridhip_comm_nranks": (ci, [vp]),
    "gridhip_comm_ctx": (vp, [vp, ci]),
    "gridhip_comm_allreduce_grids": (ci, [vp, i64, C.POINTER(vp)]),
    "gridhip_comm_allreduce_grid": (ci, [vp, i64, vp]),
    "gridhip_comm_allreduce_rows": (ci, [vp, i64, i64, i64, C.POINTER(vp)]),
    "gridhip_comm_allreduce_grid_rows": (ci, [vp, i64, i64, i64, vp]),
    "gridhip_comm_set_option": (ci, [vp, C.c_char_p, i64]),
    "gridhip_comm_get_option": (ci, [vp, C.c_char_p, C.POINTER(i64)]),
    "gridhip_comm_set_stream": (ci, [vp, ci, vp]),
    "gridhip_comm_reset_stream": (ci, [vp, ci]),
    "gridhip_comm_convgrid2": (ci, [vp] + _CONV2_DEV[1:]),
    "gridhip_malloc": (ci, [vp, C.POINTER(vp), i64]),
    "gridhip_free": (ci, [vp, vp]),
    "gridhip_memcpy_h2d": (ci, [vp, vp, vp, i64]),
    "gridhip_memcpy_d2h": (ci, [vp, vp, vp, i64]),
    "gridhip_memset": (ci, [vp, vp, ci, i64]),
    "gridhip_last_timing": (ci, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gridhip_timing": (ci, [vp, ci, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gridhip_enable_timing": (ci, [vp, ci]),
}

# per entry point, which arguments after the handle it takes by address (arrays; NULL allowed where the header says so)
POINTERS = {name: tuple(i - 1 for i, t in enumerate(args) if t is vp and i > 0) for name, (_, args) in SIGNATURES.items()}

_lib = None


class GridHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gridhip error {code}: {msg}")
        self.code = code


def load():
    """Load libgridhip.so and attach prototypes.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ska-sdp-accelerate-gridding_amd/csrc`). There is no CPU fallback."
        )
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 and loads
    # it by path, so a system copy loaded first would leave torch a second runtime that finds
    # no GPUs.  Importing torch first makes libgridhip's NEEDED libamdhip64.so.7 resolve (by
    # SONAME) to the copy torch uses.  Callers without torch (C, Haskell) get the system one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
