{-# LANGUAGE ForeignFunctionInterface #-}
{-# LANGUAGE ScopedTypeVariables #-}
-- |
-- GridHip: binding of libgridhip.so (include/gridhip.h), the MI355X-native gridders behind the signatures of
-- src/Gridding.hs.  A maintainer of sakehl/SKA-SDP-Accelerate-gridding adds this file as src/GridHip.hs (cabal:
-- other-modules GridHip, extra-libraries gridhip) and replaces the bodies of grid / convgrid / convgrid2 /
-- convgrid3 / convgrid4 as Gridding.patch.md shows; every signature of src/Gridding.hs stays as it is.
--
-- Style and conventions are those of the reference's own binding, src/Hdf5.hs:30-67,113-137:
--   * foreign import ccall, plain pointers and integers, the CALLER allocates outputs (mallocForeignPtrArray here,
--     mallocArray + newForeignPtr finalizerFree there);
--   * Accelerate arrays cross without a copy through accelerate-io (toForeignPtrs / fromForeignPtrs): a
--     Vector (F,F,F) is three buffers, an array of Complex Double ONE interleaved (re,im) buffer
--     (src/Hdf5.hs:113-137 adopts such a buffer as a single ForeignPtr; hdf5/hdf5.cc:14-17 is struct {double r, i;});
--   * shapes travel as plain integers in C order (row-major [y][x] grids, [W][Q][Q][gh][gw] kernel tables).
-- One deliberate departure: every entry point returns a status and `check` turns a failure into `error` with the
-- library's message, where the reference's shim drops HDF5 statuses (hdf5/hdf5.cc:62,70,159).
--
-- STATUS: there is no GHC in the image this library is built and tested in, so this module has never been compiled.
-- The `foreign import` block is generated from include/gridhip.h (bindings/haskell/gen_imports.py) and
-- tests/test_haskell_shim.py checks names, arity and C types of every import against the header; the wrappers below
-- it are written by hand in the idiom of src/Hdf5.hs.
module GridHip
  ( GridHip, withGridHip, openGridHip, closeGridHip, setOption, getOption
  -- * gridders (IO forms of src/Gridding.hs:95-98, 153-157, 199-204, 246-252, 318-324)
  , gridIO, convgridIO, convgrid2IO, degrid2IO, awgridIO, awdegridIO
  -- * imaging functions and do_imaging (src/Gridding.hs:76-93, 115-124, 399-449, 452-478, 509-549)
  , simpleImagingIO, convImagingIO, wCacheImagingIO, awImagingIO, doImagingIO, ImagingKind(..)
  -- * prediction: a model image -> visibilities, the other half of a major cycle (absent from the reference)
  , predictIO
  -- * imagers: the baselines of a major cycle bound once, one call per cycle (include/gridhip.h, gridhip_imager_*)
  , ImagerH, withImager, imagerCycleIO
  -- * deconvolution: Hogbom CLEAN, alone or inside an imager's major-cycle loop (absent from the reference)
  , CleanOptions(..), cleanIO, imagerCleanIO, imagerDeconvolveIO
  -- * multi-scale CLEAN: the same with components of several scales (absent from the reference)
  , mscleanIO, imagerMscleanIO, imagerMsDeconvolveIO, msDefaultBias
  -- * clean masks and noise-based stop levels: robust image statistics and the _auto forms (absent from the reference)
  , AutoOptions(..), imageStatsIO, cleanAutoIO, imagerDeconvolveAutoIO
  -- * auto-masking: the clean mask from the map itself, alone or inside the major-cycle loop (absent from the reference)
  , AutomaskOptions(..), automaskIO, imagerDeconvolveAutomaskIO
  -- * wide-band imaging: Taylor-term major cycles and the multi-term CLEAN (absent from the reference)
  , mfcleanIO, imagerSetSpectralIO, imagerMfsCycleIO, imagerMfDeconvolveIO
  -- * joint deconvolution: P images of one sky - Stokes planes, channels - cleaned at shared positions (absent from the reference)
  , JointMetric(..), jcleanIO
  -- * the restoring beam fitted to a PSF, and model * beam + residual (absent from the reference)
  , fitBeamIO, restoreIO, imagerBeamIO, imagerRestoreIO
  -- * imaging weights: natural, uniform, Briggs, taper and data weights, alone or as what an imager is created with
  , Weighting(..), WeightMode(..), weightsIO, imagerCreateWeightedIO, imagerCreateAwWeightedIO, imagerDestroyIO
  , imagerWeightStatsIO
  , GainSolve(..), gaincalIO, applyGainsIO, imagerSelfcalIO
  , ddcalIO, ddSubtractIO, imagerPeelIO
  -- * polarisation: 2x2 Jones matrices per antenna, their application, correlations <-> Stokes (absent from the reference)
  , JonesMode(..), jonescalIO, applyJonesIO, stokesIO
  , FlagOptions(..), flagResidualsIO
  , dftPredictIO, componentsFromImageIO
  , findSourcesIO
  -- * the reference's one wired-up program after its HDF5 reads (src/ImageDataset.hs:54-77) as one call
  , awGriddingIO
  -- * a whole node (single process, all devices; RCCL all-reduce of the partial grids)
  , Node, withNode, convgrid2NodeIO
  ) where

import Foreign
import Foreign.C.Types
import Foreign.C.String
import Control.Exception (bracket)
import Control.Monad (when)

import qualified Data.Array.Accelerate                       as A
import qualified Data.Array.Accelerate.Array.Sugar           as A hiding (shape)
import qualified Data.Array.Accelerate.IO.Foreign.ForeignPtr as A
import Data.Array.Accelerate.Data.Complex

import Types   -- F, Visibility, BaseLine, BaseLines, Antenna (src/Types.hs:7-16)

data Ctx
data Plan
data AwPlan
data Imager
data WStack
data Comm
newtype GridHip = GridHip (Ptr Ctx)
newtype Node    = Node (Ptr Comm)

-- ---------------------------------------------------------------------------------------------------------
-- foreign imports: generated from include/gridhip.h by bindings/haskell/gen_imports.py - do not edit by hand
-- BEGIN GENERATED IMPORTS
-- int gridhip_version()
foreign import ccall unsafe "gridhip_version"
  c_version :: IO CInt
-- const char * gridhip_strerror(code)
foreign import ccall unsafe "gridhip_strerror"
  c_strerror :: CInt -> IO CString
-- int gridhip_device_count(count)
foreign import ccall unsafe "gridhip_device_count"
  c_device_count :: Ptr CInt -> IO CInt
-- int gridhip_create(device, ctx)
foreign import ccall unsafe "gridhip_create"
  c_create :: CInt -> Ptr (Ptr Ctx) -> IO CInt
-- int gridhip_destroy(ctx)
foreign import ccall unsafe "gridhip_destroy"
  c_destroy :: Ptr Ctx -> IO CInt
-- const char * gridhip_last_error(ctx)
foreign import ccall unsafe "gridhip_last_error"
  c_last_error :: Ptr Ctx -> IO CString
-- int gridhip_set_stream(ctx, hip_stream)
foreign import ccall unsafe "gridhip_set_stream"
  c_set_stream :: Ptr Ctx -> Ptr () -> IO CInt
-- int gridhip_reset_stream(ctx)
foreign import ccall unsafe "gridhip_reset_stream"
  c_reset_stream :: Ptr Ctx -> IO CInt
-- void * gridhip_get_stream(ctx)
foreign import ccall unsafe "gridhip_get_stream"
  c_get_stream :: Ptr Ctx -> IO (Ptr ())
-- int gridhip_synchronize(ctx)
foreign import ccall unsafe "gridhip_synchronize"
  c_synchronize :: Ptr Ctx -> IO CInt
-- int gridhip_set_option(ctx, key, value)
foreign import ccall unsafe "gridhip_set_option"
  c_set_option :: Ptr Ctx -> CString -> Int64 -> IO CInt
-- int gridhip_get_option(ctx, key, value)
foreign import ccall unsafe "gridhip_get_option"
  c_get_option :: Ptr Ctx -> CString -> Ptr Int64 -> IO CInt
-- int gridhip_last_dropped(ctx, dropped)
foreign import ccall unsafe "gridhip_last_dropped"
  c_last_dropped :: Ptr Ctx -> Ptr Int64 -> IO CInt
-- int gridhip_grid(ctx, H, Wd, grid, n, u, v, uv_stride, vis)
foreign import ccall unsafe "gridhip_grid"
  c_grid :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_convgrid(ctx, H, Wd, grid, n, Q, gh, gw, gcf, u, v, uv_stride, vis)
foreign import ccall unsafe "gridhip_convgrid"
  c_convgrid :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_convgrid2(ctx, H, Wd, grid, n, W, Q, gh, gw, gcf, u, v, uv_stride, wbin, vis)
foreign import ccall unsafe "gridhip_convgrid2"
  c_convgrid2 :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_degrid2(ctx, H, Wd, grid, n, W, Q, gh, gw, gcf, u, v, uv_stride, wbin, vis_out)
foreign import ccall unsafe "gridhip_degrid2"
  c_degrid2 :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_grid_dev(ctx, H, Wd, grid, n, u, v, uv_stride, vis)
foreign import ccall unsafe "gridhip_grid_dev"
  c_grid_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_convgrid_dev(ctx, H, Wd, grid, n, Q, gh, gw, gcf, u, v, uv_stride, vis)
foreign import ccall unsafe "gridhip_convgrid_dev"
  c_convgrid_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_convgrid2_dev(ctx, H, Wd, grid, n, W, Q, gh, gw, gcf, u, v, uv_stride, wbin, vis)
foreign import ccall unsafe "gridhip_convgrid2_dev"
  c_convgrid2_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_degrid2_dev(ctx, H, Wd, grid, n, W, Q, gh, gw, gcf, u, v, uv_stride, wbin, vis_out)
foreign import ccall unsafe "gridhip_degrid2_dev"
  c_degrid2_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_plan_create_dev(ctx, H, Wd, n, W, Q, gh, gw, u, v, uv_stride, wbin, plan)
foreign import ccall unsafe "gridhip_plan_create_dev"
  c_plan_create_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr (Ptr Plan) -> IO CInt
-- int gridhip_plan_grid_dev(plan, gcf, vis, grid)
foreign import ccall unsafe "gridhip_plan_grid_dev"
  c_plan_grid_dev :: Ptr Plan -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_plan_degrid_dev(plan, gcf, grid, vis_out)
foreign import ccall unsafe "gridhip_plan_degrid_dev"
  c_plan_degrid_dev :: Ptr Plan -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_plan_destroy(plan)
foreign import ccall unsafe "gridhip_plan_destroy"
  c_plan_destroy :: Ptr Plan -> IO CInt
-- int64_t gridhip_image_size(theta, lam)
foreign import ccall unsafe "gridhip_image_size"
  c_image_size :: CDouble -> Int64 -> IO Int64
-- int gridhip_wbins(ctx, n, w, wstep, wbin, wmin, nplanes)
foreign import ccall unsafe "gridhip_wbins"
  c_wbins :: Ptr Ctx -> Int64 -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> IO CInt
-- int gridhip_find_closest(ctx, nws, ws, n, w, out)
foreign import ccall unsafe "gridhip_find_closest"
  c_find_closest :: Ptr Ctx -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr Int64 -> IO CInt
-- int gridhip_mirror_uvw(ctx, n, u, v, w, vis)
foreign import ccall unsafe "gridhip_mirror_uvw"
  c_mirror_uvw :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_doweight(ctx, theta, lam, n, u, v, vis)
foreign import ccall unsafe "gridhip_doweight"
  c_doweight :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_make_grid_hermitian(ctx, N, grid)
foreign import ccall unsafe "gridhip_make_grid_hermitian"
  c_make_grid_hermitian :: Ptr Ctx -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_fft2_centered(ctx, N, in, out, inverse)
foreign import ccall unsafe "gridhip_fft2_centered"
  c_fft2_centered :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> CInt -> IO CInt
-- int gridhip_w_kernel(ctx, theta, w, npixFF, npixKern, qpx, out)
foreign import ccall unsafe "gridhip_w_kernel"
  c_w_kernel :: Ptr Ctx -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_simple_imaging(ctx, theta, lam, n, u, v, uv_stride, vis, grid)
foreign import ccall unsafe "gridhip_simple_imaging"
  c_simple_imaging :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_conv_imaging(ctx, Q, gh, gw, kv, theta, lam, n, u, v, uv_stride, vis, grid)
foreign import ccall unsafe "gridhip_conv_imaging"
  c_conv_imaging :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_w_cache_imaging(ctx, wstep, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, grid)
foreign import ccall unsafe "gridhip_w_cache_imaging"
  c_w_cache_imaging :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_awgrid(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis)
foreign import ccall unsafe "gridhip_awgrid"
  c_awgrid :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_awgrid_dev(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis)
foreign import ccall unsafe "gridhip_awgrid_dev"
  c_awgrid_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_aw_last_stats(ctx, vis_keyed, kernels_built)
foreign import ccall unsafe "gridhip_aw_last_stats"
  c_aw_last_stats :: Ptr Ctx -> Ptr Int64 -> Ptr Int64 -> IO CInt
-- int gridhip_awdegrid(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis_out)
foreign import ccall unsafe "gridhip_awdegrid"
  c_awdegrid :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_awdegrid_dev(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis_out)
foreign import ccall unsafe "gridhip_awdegrid_dev"
  c_awdegrid_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_aw_plan_create_dev(ctx, H, Wd, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, plan)
foreign import ccall unsafe "gridhip_aw_plan_create_dev"
  c_aw_plan_create_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr (Ptr AwPlan) -> IO CInt
-- int gridhip_aw_plan_grid_dev(plan, vis, grid)
foreign import ccall unsafe "gridhip_aw_plan_grid_dev"
  c_aw_plan_grid_dev :: Ptr AwPlan -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_aw_plan_degrid_dev(plan, grid, vis_out)
foreign import ccall unsafe "gridhip_aw_plan_degrid_dev"
  c_aw_plan_degrid_dev :: Ptr AwPlan -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_aw_plan_destroy(plan)
foreign import ccall unsafe "gridhip_aw_plan_destroy"
  c_aw_plan_destroy :: Ptr AwPlan -> IO CInt
-- int gridhip_aw_imaging(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, grid)
foreign import ccall unsafe "gridhip_aw_imaging"
  c_aw_imaging :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_aw_imaging_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, grid)
foreign import ccall unsafe "gridhip_aw_imaging_dev"
  c_aw_imaging_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_do_imaging_aw(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging_aw"
  c_do_imaging_aw :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_do_imaging_aw_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging_aw_dev"
  c_do_imaging_aw_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_aw_gridding(ctx, theta, lam, f, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, image, imax)
foreign import ccall unsafe "gridhip_aw_gridding"
  c_aw_gridding :: Ptr Ctx -> CDouble -> Int64 -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_aw_gridding_dev(ctx, theta, lam, f, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis, image, imax)
foreign import ccall unsafe "gridhip_aw_gridding_dev"
  c_aw_gridding_dev :: Ptr Ctx -> CDouble -> Int64 -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_do_imaging(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, n, u, v, w, uv_stride, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging"
  c_do_imaging :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_do_imaging_dev(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, n, u, v, w, uv_stride, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging_dev"
  c_do_imaging_dev :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_w_cache_imaging_dev(ctx, wstep, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, grid)
foreign import ccall unsafe "gridhip_w_cache_imaging_dev"
  c_w_cache_imaging_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, model, n, u, v, w, uv_stride, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict"
  c_predict :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict_dev(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, model, n, u, v, w, uv_stride, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict_dev"
  c_predict_dev :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict_aw(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, model, n, u, v, w, uv_stride, a1, a2, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict_aw"
  c_predict_aw :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict_aw_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, model, n, u, v, w, uv_stride, a1, a2, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict_aw_dev"
  c_predict_aw_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_create_dev(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, n, u, v, w, uv_stride, imager)
foreign import ccall unsafe "gridhip_imager_create_dev"
  c_imager_create_dev :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr (Ptr Imager) -> IO CInt
-- int gridhip_imager_create_aw_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, imager)
foreign import ccall unsafe "gridhip_imager_create_aw_dev"
  c_imager_create_aw_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr (Ptr Imager) -> IO CInt
-- int gridhip_imager_psf_dev(imager, psf, pmax)
foreign import ccall unsafe "gridhip_imager_psf_dev"
  c_imager_psf_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_cycle_dev(imager, model, vis, image, vis_res)
foreign import ccall unsafe "gridhip_imager_cycle_dev"
  c_imager_cycle_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_predict_dev(imager, model, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_imager_predict_dev"
  c_imager_predict_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_destroy(imager)
foreign import ccall unsafe "gridhip_imager_destroy"
  c_imager_destroy :: Ptr Imager -> IO CInt
-- int gridhip_clean(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_clean"
  c_clean :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_clean_dev(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_clean_dev"
  c_clean_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_clean_dev(imager, residual, model, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_clean_dev"
  c_imager_clean_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_deconvolve_dev(imager, vis, model, image, nmajor, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_deconvolve_dev"
  c_imager_deconvolve_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_msclean(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_msclean"
  c_msclean :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_msclean_dev(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_msclean_dev"
  c_msclean_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_msclean_dev(imager, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_msclean_dev"
  c_imager_msclean_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_msdeconvolve_dev(imager, vis, model, image, nmajor, S, scales, bias, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_msdeconvolve_dev"
  c_imager_msdeconvolve_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_image_stats(ctx, N, image, mask, border, stats)
foreign import ccall unsafe "gridhip_image_stats"
  c_image_stats :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_image_stats_dev(ctx, N, image, mask, border, stats)
foreign import ccall unsafe "gridhip_image_stats_dev"
  c_image_stats_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_image_stats_dev(imager, image, mask, border, stats)
foreign import ccall unsafe "gridhip_imager_image_stats_dev"
  c_imager_image_stats_dev :: Ptr Imager -> Ptr CDouble -> Ptr Word8 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_clean_auto(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_clean_auto"
  c_clean_auto :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_clean_auto_dev(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_clean_auto_dev"
  c_clean_auto_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_msclean_auto(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_msclean_auto"
  c_msclean_auto :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_msclean_auto_dev(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_msclean_auto_dev"
  c_msclean_auto_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_clean_auto_dev(imager, residual, model, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_imager_clean_auto_dev"
  c_imager_clean_auto_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_msclean_auto_dev(imager, residual, model, S, scales, bias, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_imager_msclean_auto_dev"
  c_imager_msclean_auto_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_deconvolve_auto_dev(imager, vis, model, image, nmajor, gain, threshold, niter, border, patch, mask, nsigma, peak_frac, stats, istats)
foreign import ccall unsafe "gridhip_imager_deconvolve_auto_dev"
  c_imager_deconvolve_auto_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_msdeconvolve_auto_dev(imager, vis, model, image, nmajor, S, scales, bias, gain, threshold, niter, border, patch, mask, nsigma, peak_frac, stats, istats)
foreign import ccall unsafe "gridhip_imager_msdeconvolve_auto_dev"
  c_imager_msdeconvolve_auto_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_automask(ctx, N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, grow, stats)
foreign import ccall unsafe "gridhip_automask"
  c_automask :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> Int64 -> CInt -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_automask_dev(ctx, N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, grow, stats)
foreign import ccall unsafe "gridhip_automask_dev"
  c_automask_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> Int64 -> CInt -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_automask_dev(imager, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, grow, stats)
foreign import ccall unsafe "gridhip_imager_automask_dev"
  c_imager_automask_dev :: Ptr Imager -> Ptr CDouble -> Ptr Word8 -> Int64 -> CInt -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_deconvolve_automask_dev(imager, vis, model, image, nmajor, gain, threshold, niter, border, patch, mask, nsigma, peak_frac_clean, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, peak_frac, min_cells, grow, stats, istats, astats)
foreign import ccall unsafe "gridhip_imager_deconvolve_automask_dev"
  c_imager_deconvolve_automask_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> CDouble -> CInt -> CDouble -> CDouble -> CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_msdeconvolve_automask_dev(imager, vis, model, image, nmajor, S, scales, bias, gain, threshold, niter, border, patch, mask, nsigma, peak_frac_clean, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, peak_frac, min_cells, grow, stats, istats, astats)
foreign import ccall unsafe "gridhip_imager_msdeconvolve_automask_dev"
  c_imager_msdeconvolve_automask_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> CDouble -> CInt -> CDouble -> CDouble -> CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int64_t gridhip_noise_map_nodes(N, border, step)
foreign import ccall unsafe "gridhip_noise_map_nodes"
  c_noise_map_nodes :: Int64 -> Int64 -> Int64 -> IO Int64
-- int gridhip_noise_map(ctx, N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, nodes, background, rms, out, stats)
foreign import ccall unsafe "gridhip_noise_map"
  c_noise_map :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> CInt -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_noise_map_dev(ctx, N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, nodes, background, rms, out, stats)
foreign import ccall unsafe "gridhip_noise_map_dev"
  c_noise_map_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Word8 -> CInt -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fit_beam(ctx, N, psf, window, cut, beam)
foreign import ccall unsafe "gridhip_fit_beam"
  c_fit_beam :: Ptr Ctx -> Int64 -> Ptr CDouble -> Int64 -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fit_beam_dev(ctx, N, psf, window, cut, beam)
foreign import ccall unsafe "gridhip_fit_beam_dev"
  c_fit_beam_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Int64 -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_restore(ctx, N, model, residual, beam, support, restored)
foreign import ccall unsafe "gridhip_restore"
  c_restore :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_restore_dev(ctx, N, model, residual, beam, support, restored)
foreign import ccall unsafe "gridhip_restore_dev"
  c_restore_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_beam_dev(imager, window, cut, beam)
foreign import ccall unsafe "gridhip_imager_beam_dev"
  c_imager_beam_dev :: Ptr Imager -> Int64 -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_restore_dev(imager, model, residual, window, cut, support, restored, beam)
foreign import ccall unsafe "gridhip_imager_restore_dev"
  c_imager_restore_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_weights(ctx, theta, lam, n, u, v, uv_stride, wt_in, mode, robust, taper_sigma, wt_out, stats)
foreign import ccall unsafe "gridhip_weights"
  c_weights :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> CInt -> CDouble -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_weights_dev(ctx, theta, lam, n, u, v, uv_stride, wt_in, mode, robust, taper_sigma, wt_out, stats)
foreign import ccall unsafe "gridhip_weights_dev"
  c_weights_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> CInt -> CDouble -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_create_weighted_dev(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, n, u, v, w, uv_stride, mode, robust, taper_sigma, wt_in, imager)
foreign import ccall unsafe "gridhip_imager_create_weighted_dev"
  c_imager_create_weighted_dev :: Ptr Ctx -> CInt -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> CInt -> CDouble -> CDouble -> Ptr CDouble -> Ptr (Ptr Imager) -> IO CInt
-- int gridhip_imager_create_aw_weighted_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, mode, robust, taper_sigma, wt_in, imager)
foreign import ccall unsafe "gridhip_imager_create_aw_weighted_dev"
  c_imager_create_aw_weighted_dev :: Ptr Ctx -> CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr Int64 -> CInt -> CDouble -> CDouble -> Ptr CDouble -> Ptr (Ptr Imager) -> IO CInt
-- int gridhip_imager_weight_stats_dev(imager, stats)
foreign import ccall unsafe "gridhip_imager_weight_stats_dev"
  c_imager_weight_stats_dev :: Ptr Imager -> Ptr CDouble -> IO CInt
-- int gridhip_mfclean(ctx, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_mfclean"
  c_mfclean :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_mfclean_dev(ctx, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_mfclean_dev"
  c_mfclean_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_set_spectral_dev(imager, T, x)
foreign import ccall unsafe "gridhip_imager_set_spectral_dev"
  c_imager_set_spectral_dev :: Ptr Imager -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_spectral_psfs_dev(imager, psfs)
foreign import ccall unsafe "gridhip_imager_spectral_psfs_dev"
  c_imager_spectral_psfs_dev :: Ptr Imager -> Ptr CDouble -> IO CInt
-- int gridhip_imager_mfs_cycle_dev(imager, models, vis, images, vis_res)
foreign import ccall unsafe "gridhip_imager_mfs_cycle_dev"
  c_imager_mfs_cycle_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_mfclean_dev(imager, residuals, models, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_mfclean_dev"
  c_imager_mfclean_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_mfdeconvolve_dev(imager, vis, models, images, nmajor, gain, threshold, niter, border, patch, stats)
foreign import ccall unsafe "gridhip_imager_mfdeconvolve_dev"
  c_imager_mfdeconvolve_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_gaincal(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_gaincal"
  c_gaincal :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_gaincal_dev(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_gaincal_dev"
  c_gaincal_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_gains(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_gains"
  c_apply_gains :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_gains_dev(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_gains_dev"
  c_apply_gains_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_selfcal_dev(imager, model, vis, A, T, a1, a2, slot, wt, mode, refant, warm, niter, tol, gains, vis_cal, wt_cal, stats)
foreign import ccall unsafe "gridhip_imager_selfcal_dev"
  c_imager_selfcal_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_ddcal(ctx, n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_ddcal"
  c_ddcal :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_ddcal_dev(ctx, n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_ddcal_dev"
  c_ddcal_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int64_t gridhip_ddcal_lds_antennas(D)
foreign import ccall unsafe "gridhip_ddcal_lds_antennas"
  c_ddcal_lds_antennas :: Int64 -> IO Int64
-- int gridhip_dd_subtract(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out)
foreign import ccall unsafe "gridhip_dd_subtract"
  c_dd_subtract :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_dd_subtract_dev(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out)
foreign import ccall unsafe "gridhip_dd_subtract_dev"
  c_dd_subtract_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_peel_dev(imager, model, vis, A, T, D, a1, a2, slot, wt, mode, refant, warm, niter, tol, model_vis, gains, vis_cal, wt_cal, stats)
foreign import ccall unsafe "gridhip_imager_peel_dev"
  c_imager_peel_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_jonescal(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_jonescal"
  c_jonescal :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_jonescal_dev(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats)
foreign import ccall unsafe "gridhip_jonescal_dev"
  c_jonescal_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> Int64 -> CInt -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int64_t gridhip_jonescal_lds_antennas()
foreign import ccall unsafe "gridhip_jonescal_lds_antennas"
  c_jonescal_lds_antennas :: IO Int64
-- int gridhip_apply_jones(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_jones"
  c_apply_jones :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_jones_dev(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_jones_dev"
  c_apply_jones_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_stokes(ctx, n, basis, which, inverse, vis, stokes)
foreign import ccall unsafe "gridhip_stokes"
  c_stokes :: Ptr Ctx -> Int64 -> CInt -> CInt -> CInt -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_stokes_dev(ctx, n, basis, which, inverse, vis, stokes)
foreign import ccall unsafe "gridhip_stokes_dev"
  c_stokes_dev :: Ptr Ctx -> Int64 -> CInt -> CInt -> CInt -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_flag_residuals(ctx, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out, group_stats, stats)
foreign import ccall unsafe "gridhip_flag_residuals"
  c_flag_residuals :: Ptr Ctx -> Int64 -> Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_flag_residuals_dev(ctx, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out, group_stats, stats)
foreign import ccall unsafe "gridhip_flag_residuals_dev"
  c_flag_residuals_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_imager_flag_dev(imager, model, vis, G, group, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out, group_stats, stats)
foreign import ccall unsafe "gridhip_imager_flag_dev"
  c_imager_flag_dev :: Ptr Imager -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_sumthreshold(ctx, B, T, F, order, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out, flags_out, baseline_stats, stats)
foreign import ccall unsafe "gridhip_sumthreshold"
  c_sumthreshold :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_sumthreshold_dev(ctx, B, T, F, order, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out, flags_out, baseline_stats, stats)
foreign import ccall unsafe "gridhip_sumthreshold_dev"
  c_sumthreshold_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_sumthreshold_tile(tile_t, tile_f)
foreign import ccall unsafe "gridhip_sumthreshold_tile"
  c_sumthreshold_tile :: Ptr Int64 -> Ptr Int64 -> IO CInt
-- int gridhip_rm_tables(ctx, C, J, lam2, weights, phi0, dphi, fwhm, tables)
foreign import ccall unsafe "gridhip_rm_tables"
  c_rm_tables :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rm_tables_dev(ctx, C, J, lam2, weights, phi0, dphi, fwhm, tables)
foreign import ccall unsafe "gridhip_rm_tables_dev"
  c_rm_tables_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rmsynth(ctx, M, C, J, tables, Q, U, cube, stats)
foreign import ccall unsafe "gridhip_rmsynth"
  c_rmsynth :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rmsynth_dev(ctx, M, C, J, tables, Q, U, cube, stats)
foreign import ccall unsafe "gridhip_rmsynth_dev"
  c_rmsynth_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rmclean(ctx, M, J, tables, cube, model, gain, threshold, niter, nsigma, noise, restore, maps, stats)
foreign import ccall unsafe "gridhip_rmclean"
  c_rmclean :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rmclean_dev(ctx, M, J, tables, cube, model, gain, threshold, niter, nsigma, noise, restore, maps, stats)
foreign import ccall unsafe "gridhip_rmclean_dev"
  c_rmclean_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_rm_tile(out)
foreign import ccall unsafe "gridhip_rm_tile"
  c_rm_tile :: Ptr Int64 -> IO CInt
-- int gridhip_contsub(ctx, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo, codes, stats)
foreign import ccall unsafe "gridhip_contsub"
  c_contsub :: Ptr Ctx -> Int64 -> Int64 -> CInt -> CInt -> CInt -> CInt -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> IO CInt
-- int gridhip_contsub_dev(ctx, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo, codes, stats)
foreign import ccall unsafe "gridhip_contsub_dev"
  c_contsub_dev :: Ptr Ctx -> Int64 -> Int64 -> CInt -> CInt -> CInt -> CInt -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Word8 -> Ptr CDouble -> IO CInt
-- int gridhip_contsub_tile(out)
foreign import ccall unsafe "gridhip_contsub_tile"
  c_contsub_tile :: Ptr Int64 -> IO CInt
-- int gridhip_fringe_tables(ctx, F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables)
foreign import ccall unsafe "gridhip_fringe_tables"
  c_fringe_tables :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_tables_dev(ctx, F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables)
foreign import ccall unsafe "gridhip_fringe_tables_dev"
  c_fringe_tables_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_search(ctx, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats)
foreign import ccall unsafe "gridhip_fringe_search"
  c_fringe_search :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_search_dev(ctx, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats)
foreign import ccall unsafe "gridhip_fringe_search_dev"
  c_fringe_search_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_solve(ctx, B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info, stats)
foreign import ccall unsafe "gridhip_fringe_solve"
  c_fringe_solve :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_solve_dev(ctx, B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info, stats)
foreign import ccall unsafe "gridhip_fringe_solve_dev"
  c_fringe_solve_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringefit(ctx, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count, min_coh2, refant, niter, tol, warm, sol, peaks, info, stats)
foreign import ccall unsafe "gridhip_fringefit"
  c_fringefit :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringefit_dev(ctx, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count, min_coh2, refant, niter, tol, warm, sol, peaks, info, stats)
foreign import ccall unsafe "gridhip_fringefit_dev"
  c_fringefit_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_fringe(ctx, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_fringe"
  c_apply_fringe :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_fringe_dev(ctx, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_fringe_dev"
  c_apply_fringe_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_fringe_tile(out)
foreign import ccall unsafe "gridhip_fringe_tile"
  c_fringe_tile :: Ptr Int64 -> IO CInt
-- int gridhip_tec_tables(ctx, F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables)
foreign import ccall unsafe "gridhip_tec_tables"
  c_tec_tables :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_tec_tables_dev(ctx, F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables)
foreign import ccall unsafe "gridhip_tec_tables_dev"
  c_tec_tables_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_tec_search(ctx, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, m0, m1, peaks, stats)
foreign import ccall unsafe "gridhip_tec_search"
  c_tec_search :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_tec_search_dev(ctx, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, m0, m1, peaks, stats)
foreign import ccall unsafe "gridhip_tec_search_dev"
  c_tec_search_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_tecfit(ctx, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count, min_coh2, refant, niter, tol, warm, sol, peaks, info, stats)
foreign import ccall unsafe "gridhip_tecfit"
  c_tecfit :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_tecfit_dev(ctx, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count, min_coh2, refant, niter, tol, warm, sol, peaks, info, stats)
foreign import ccall unsafe "gridhip_tecfit_dev"
  c_tecfit_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> CDouble -> Int64 -> Int64 -> CDouble -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_tec(ctx, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_tec"
  c_apply_tec :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_apply_tec_dev(ctx, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out)
foreign import ccall unsafe "gridhip_apply_tec_dev"
  c_apply_tec_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr Int64 -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_tec_tile(out)
foreign import ccall unsafe "gridhip_tec_tile"
  c_tec_tile :: Ptr Int64 -> IO CInt
-- int gridhip_dft_predict(ctx, C, comps, count, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats)
foreign import ccall unsafe "gridhip_dft_predict"
  c_dft_predict :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Int64 -> CInt -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_dft_predict_dev(ctx, C, comps, count_dev, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats)
foreign import ccall unsafe "gridhip_dft_predict_dev"
  c_dft_predict_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr Int64 -> CInt -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_components_from_image(ctx, theta, lam, T, model, max_c, comps, count)
foreign import ccall unsafe "gridhip_components_from_image"
  c_components_from_image :: Ptr Ctx -> CDouble -> Int64 -> CInt -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr Int64 -> IO CInt
-- int gridhip_components_from_image_dev(ctx, theta, lam, T, model, max_c, comps, count)
foreign import ccall unsafe "gridhip_components_from_image_dev"
  c_components_from_image_dev :: Ptr Ctx -> CDouble -> Int64 -> CInt -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr Int64 -> IO CInt
-- int gridhip_find_sources(ctx, theta, lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam, correct, max_c, comps, info, count, stats)
foreign import ccall unsafe "gridhip_find_sources"
  c_find_sources :: Ptr Ctx -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> CInt -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_find_sources_dev(ctx, theta, lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam, correct, max_c, comps, info, count, stats)
foreign import ccall unsafe "gridhip_find_sources_dev"
  c_find_sources_dev :: Ptr Ctx -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> CInt -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_imager_find_sources_dev(imager, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam, correct, max_c, comps, info, count, stats)
foreign import ccall unsafe "gridhip_imager_find_sources_dev"
  c_imager_find_sources_dev :: Ptr Imager -> Ptr CDouble -> Int64 -> CDouble -> CDouble -> CDouble -> CDouble -> Ptr CDouble -> CDouble -> Int64 -> Ptr CDouble -> CInt -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_phase_shift(ctx, n, R, u, v, w, uv_stride, vis_in, vis_out, u_out, v_out, w_out, out_stride, stats)
foreign import ccall unsafe "gridhip_phase_shift"
  c_phase_shift :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_phase_shift_dev(ctx, n, R, u, v, w, uv_stride, vis_in, vis_out, u_out, v_out, w_out, out_stride, stats)
foreign import ccall unsafe "gridhip_phase_shift_dev"
  c_phase_shift_dev :: Ptr Ctx -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_average(ctx, n, G, group, R, u, v, w, uv_stride, x, vis, wt, u_out, v_out, w_out, out_stride, x_out, vis_out, wt_out, count_out, stats)
foreign import ccall unsafe "gridhip_average"
  c_average :: Ptr Ctx -> Int64 -> Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_average_dev(ctx, n, G, group, R, u, v, w, uv_stride, x, vis, wt, u_out, v_out, w_out, out_stride, x_out, vis_out, wt_out, count_out, stats)
foreign import ccall unsafe "gridhip_average_dev"
  c_average_dev :: Ptr Ctx -> Int64 -> Int64 -> Ptr Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_mosaic(ctx, F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out, wsum, stats)
foreign import ccall unsafe "gridhip_mosaic"
  c_mosaic :: Ptr Ctx -> Int64 -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> CInt -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_mosaic_dev(ctx, F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out, wsum, stats)
foreign import ccall unsafe "gridhip_mosaic_dev"
  c_mosaic_dev :: Ptr Ctx -> Int64 -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> CInt -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_reproject(ctx, Ns, theta_s, image, R, kind, inner, outer, blank, Nd, theta_d, out)
foreign import ccall unsafe "gridhip_reproject"
  c_reproject :: Ptr Ctx -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_reproject_dev(ctx, Ns, theta_s, image, R, kind, inner, outer, blank, Nd, theta_d, out)
foreign import ccall unsafe "gridhip_reproject_dev"
  c_reproject_dev :: Ptr Ctx -> Int64 -> CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> CDouble -> Int64 -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_wstack_create_dev(ctx, wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, ws)
foreign import ccall unsafe "gridhip_wstack_create_dev"
  c_wstack_create_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr (Ptr WStack) -> IO CInt
-- int gridhip_wstack_image_dev(ws, vis, image)
foreign import ccall unsafe "gridhip_wstack_image_dev"
  c_wstack_image_dev :: Ptr WStack -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_wstack_predict_dev(ws, model, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_wstack_predict_dev"
  c_wstack_predict_dev :: Ptr WStack -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_wstack_info(ws, layers, occupied, pmin, dropped)
foreign import ccall unsafe "gridhip_wstack_info"
  c_wstack_info :: Ptr WStack -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> IO CInt
-- int gridhip_wstack_destroy(ws)
foreign import ccall unsafe "gridhip_wstack_destroy"
  c_wstack_destroy :: Ptr WStack -> IO CInt
-- int gridhip_do_imaging_wstack(ctx, wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging_wstack"
  c_do_imaging_wstack :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_do_imaging_wstack_dev(ctx, wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, image, psf, pmax)
foreign import ccall unsafe "gridhip_do_imaging_wstack_dev"
  c_do_imaging_wstack_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict_wstack(ctx, wstep, M, qpx, npixFF, npixKern, theta, lam, model, n, u, v, w, uv_stride, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict_wstack"
  c_predict_wstack :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_predict_wstack_dev(ctx, wstep, M, qpx, npixFF, npixKern, theta, lam, model, n, u, v, w, uv_stride, vis_sub, vis_out)
foreign import ccall unsafe "gridhip_predict_wstack_dev"
  c_predict_wstack_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> CDouble -> Int64 -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_jclean(ctx, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_jclean"
  c_jclean :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_jclean_dev(ctx, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch, mask, nsigma, noise, peak_frac, stats)
foreign import ccall unsafe "gridhip_jclean_dev"
  c_jclean_dev :: Ptr Ctx -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> CInt -> CDouble -> CDouble -> Int64 -> Int64 -> Int64 -> Ptr Word8 -> CDouble -> Ptr CDouble -> CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_comm_create(ndev, dev_ids, comm)
foreign import ccall safe "gridhip_comm_create"
  c_comm_create :: CInt -> Ptr CInt -> Ptr (Ptr Comm) -> IO CInt
-- int gridhip_comm_unique_id(id128)
foreign import ccall unsafe "gridhip_comm_unique_id"
  c_comm_unique_id :: Ptr () -> IO CInt
-- int gridhip_comm_create_rank(ctx, nranks, rank, id128, comm)
foreign import ccall safe "gridhip_comm_create_rank"
  c_comm_create_rank :: Ptr Ctx -> CInt -> CInt -> Ptr () -> Ptr (Ptr Comm) -> IO CInt
-- int gridhip_comm_destroy(comm)
foreign import ccall safe "gridhip_comm_destroy"
  c_comm_destroy :: Ptr Comm -> IO CInt
-- const char * gridhip_comm_last_error(comm)
foreign import ccall unsafe "gridhip_comm_last_error"
  c_comm_last_error :: Ptr Comm -> IO CString
-- int gridhip_comm_ndev(comm)
foreign import ccall unsafe "gridhip_comm_ndev"
  c_comm_ndev :: Ptr Comm -> IO CInt
-- int gridhip_comm_nranks(comm)
foreign import ccall unsafe "gridhip_comm_nranks"
  c_comm_nranks :: Ptr Comm -> IO CInt
-- gridhip_ctx * gridhip_comm_ctx(comm, i)
foreign import ccall unsafe "gridhip_comm_ctx"
  c_comm_ctx :: Ptr Comm -> CInt -> IO (Ptr Ctx)
-- int gridhip_comm_allreduce_grids(comm, cells, grids)
foreign import ccall unsafe "gridhip_comm_allreduce_grids"
  c_comm_allreduce_grids :: Ptr Comm -> Int64 -> Ptr (Ptr CDouble) -> IO CInt
-- int gridhip_comm_allreduce_grid(comm, cells, grid)
foreign import ccall unsafe "gridhip_comm_allreduce_grid"
  c_comm_allreduce_grid :: Ptr Comm -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_comm_allreduce_rows(comm, Wd, y0, y1, grids)
foreign import ccall unsafe "gridhip_comm_allreduce_rows"
  c_comm_allreduce_rows :: Ptr Comm -> Int64 -> Int64 -> Int64 -> Ptr (Ptr CDouble) -> IO CInt
-- int gridhip_comm_allreduce_grid_rows(comm, Wd, y0, y1, grid)
foreign import ccall unsafe "gridhip_comm_allreduce_grid_rows"
  c_comm_allreduce_grid_rows :: Ptr Comm -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_comm_set_option(comm, key, value)
foreign import ccall unsafe "gridhip_comm_set_option"
  c_comm_set_option :: Ptr Comm -> CString -> Int64 -> IO CInt
-- int gridhip_comm_get_option(comm, key, value)
foreign import ccall unsafe "gridhip_comm_get_option"
  c_comm_get_option :: Ptr Comm -> CString -> Ptr Int64 -> IO CInt
-- int gridhip_comm_set_stream(comm, i, hip_stream)
foreign import ccall unsafe "gridhip_comm_set_stream"
  c_comm_set_stream :: Ptr Comm -> CInt -> Ptr () -> IO CInt
-- int gridhip_comm_reset_stream(comm, i)
foreign import ccall unsafe "gridhip_comm_reset_stream"
  c_comm_reset_stream :: Ptr Comm -> CInt -> IO CInt
-- int gridhip_comm_convgrid2(comm, H, Wd, grid, n, W, Q, gh, gw, gcf, u, v, uv_stride, wbin, vis)
foreign import ccall safe "gridhip_comm_convgrid2"
  c_comm_convgrid2 :: Ptr Comm -> Int64 -> Int64 -> Ptr CDouble -> Int64 -> Int64 -> Int64 -> Int64 -> Int64 -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> Int64 -> Ptr Int64 -> Ptr CDouble -> IO CInt
-- int gridhip_malloc(ctx, dptr, bytes)
foreign import ccall unsafe "gridhip_malloc"
  c_malloc :: Ptr Ctx -> Ptr (Ptr ()) -> Int64 -> IO CInt
-- int gridhip_free(ctx, dptr)
foreign import ccall unsafe "gridhip_free"
  c_free :: Ptr Ctx -> Ptr () -> IO CInt
-- int gridhip_memcpy_h2d(ctx, dst, src, bytes)
foreign import ccall unsafe "gridhip_memcpy_h2d"
  c_memcpy_h2d :: Ptr Ctx -> Ptr () -> Ptr () -> Int64 -> IO CInt
-- int gridhip_memcpy_d2h(ctx, dst, src, bytes)
foreign import ccall unsafe "gridhip_memcpy_d2h"
  c_memcpy_d2h :: Ptr Ctx -> Ptr () -> Ptr () -> Int64 -> IO CInt
-- int gridhip_memset(ctx, dptr, value, bytes)
foreign import ccall unsafe "gridhip_memset"
  c_memset :: Ptr Ctx -> Ptr () -> CInt -> Int64 -> IO CInt
-- int gridhip_last_timing(ctx, ms_total, ms_prepass, ms_kernel)
foreign import ccall unsafe "gridhip_last_timing"
  c_last_timing :: Ptr Ctx -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_timing(ctx, back, ms_total, ms_prepass, ms_kernel)
foreign import ccall unsafe "gridhip_timing"
  c_timing :: Ptr Ctx -> CInt -> Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO CInt
-- int gridhip_enable_timing(ctx, enable)
foreign import ccall unsafe "gridhip_enable_timing"
  c_enable_timing :: Ptr Ctx -> CInt -> IO CInt
-- END GENERATED IMPORTS
-- ---------------------------------------------------------------------------------------------------------

fi :: (Integral a, Num b) => a -> b
fi = fromIntegral

-- | a context on HIP device `dev` (one device, one stream; not thread-safe: one per calling thread)
openGridHip :: Int -> IO GridHip
openGridHip dev = alloca $ \pp -> do
  rc <- c_create (fi dev) pp
  when (rc /= 0) $ c_strerror rc >>= peekCString >>= \m -> error ("gridhip_create: " ++ m)
  GridHip <$> peek pp

closeGridHip :: GridHip -> IO ()
closeGridHip (GridHip p) = () <$ c_destroy p

withGridHip :: Int -> (GridHip -> IO a) -> IO a
withGridHip dev = bracket (openGridHip dev) closeGridHip

check :: GridHip -> CInt -> IO ()
check (GridHip p) rc = when (rc /= 0) $ do
  msg <- c_last_error p >>= peekCString
  error ("gridhip (" ++ show rc ++ "): " ++ msg)

setOption :: GridHip -> String -> Int -> IO ()
setOption h@(GridHip p) key val = withCString key $ \k -> c_set_option p k (fi val) >>= check h

getOption :: GridHip -> String -> IO Int
getOption h@(GridHip p) key = withCString key $ \k -> alloca $ \o -> do
  c_get_option p k o >>= check h
  fi <$> peek o

-- Pointer views of Accelerate arrays (no copy).  Complex Double arrays are one interleaved buffer of doubles; a
-- Vector (F,F,F) is three buffers, a Vector (Int,Int,Int) likewise.
withCplx :: A.Shape sh => A.Array sh Visibility -> (Ptr CDouble -> IO b) -> IO b
withCplx arr k = withForeignPtr (castForeignPtr (A.toForeignPtrs arr)) k

withF :: A.Shape sh => A.Array sh F -> (Ptr CDouble -> IO b) -> IO b
withF arr k = withForeignPtr (castForeignPtr (A.toForeignPtrs arr)) k

withI :: A.Shape sh => A.Array sh Int -> (Ptr Int64 -> IO b) -> IO b
withI arr k = withForeignPtr (castForeignPtr (A.toForeignPtrs arr)) k

withI64 :: A.Shape sh => A.Array sh Antenna -> (Ptr Int64 -> IO b) -> IO b
withI64 arr k = withForeignPtr (castForeignPtr (A.toForeignPtrs arr)) k

withUVW :: A.Vector BaseLines -> (Ptr CDouble -> Ptr CDouble -> Ptr CDouble -> IO b) -> IO b
withUVW p k =
  let ((((), pu), pv), pw) = A.toForeignPtrs p
  in withForeignPtr (castForeignPtr pu) $ \u -> withForeignPtr (castForeignPtr pv) $ \v ->
     withForeignPtr (castForeignPtr pw) $ \w -> k u v w

withIdx3 :: A.Vector (Int, Int, Int) -> (Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> IO b) -> IO b
withIdx3 ix k =
  let ((((), p0), p1), p2) = A.toForeignPtrs ix
  in withForeignPtr (castForeignPtr p0) $ \a -> withForeignPtr (castForeignPtr p1) $ \b ->
     withForeignPtr (castForeignPtr p2) $ \c -> k a b c

-- a fresh copy of the destination grid: every gridder ACCUMULATES INTO the grid it is given, as
-- `permute (+) a ...` does (src/Gridding.hs:99,197,244), and Accelerate arrays are immutable
copyGrid :: A.Matrix Visibility -> IO (ForeignPtr CDouble, Int, Int)
copyGrid a = do
  let A.Z A.:. hgt A.:. wid = A.arrayShape a
  out <- mallocForeignPtrArray (2 * hgt * wid)
  withForeignPtr out $ \o -> withCplx a $ \src -> copyArray o src (2 * hgt * wid)
  return (out, hgt, wid)

adoptGrid :: ForeignPtr CDouble -> Int -> Int -> A.Matrix Visibility
adoptGrid out hgt wid = A.fromForeignPtrs (A.Z A.:. hgt A.:. wid) (castForeignPtr out)

newGrid :: Int -> IO (ForeignPtr CDouble)
newGrid n = mallocForeignPtrArray (2 * n * n)

-- | grid a p v  (src/Gridding.hs:95-98)
gridIO :: GridHip -> A.Matrix Visibility -> A.Vector BaseLines -> A.Vector Visibility -> IO (A.Matrix Visibility)
gridIO h@(GridHip c) a p v = do
  (out, hgt, wid) <- copyGrid a
  let A.Z A.:. n = A.arrayShape v
  withForeignPtr out $ \o -> withUVW p $ \pu pv _ -> withCplx v $ \vs ->
    c_grid c (fi hgt) (fi wid) o (fi n) pu pv 1 vs >>= check h
  return (adoptGrid out hgt wid)

-- | convgrid gcf a p v  (src/Gridding.hs:153-157); gcf is [Q,Q,gh,gw]
convgridIO :: GridHip -> A.Array A.DIM4 Visibility -> A.Matrix Visibility -> A.Vector BaseLines
           -> A.Vector Visibility -> IO (A.Matrix Visibility)
convgridIO h@(GridHip c) gcf a p v = do
  (out, hgt, wid) <- copyGrid a
  let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape gcf
      A.Z A.:. n = A.arrayShape v
  withForeignPtr out $ \o -> withCplx gcf $ \k -> withUVW p $ \pu pv _ -> withCplx v $ \vs ->
    c_convgrid c (fi hgt) (fi wid) o (fi n) (fi q) (fi gh) (fi gw) k pu pv 1 vs >>= check h
  return (adoptGrid out hgt wid)

-- | convgrid2 gcf a p wbin v  (src/Gridding.hs:199-204); gcf is [W,Q,Q,gh,gw]
convgrid2IO :: GridHip -> A.Array A.DIM5 Visibility -> A.Matrix Visibility -> A.Vector BaseLines
            -> A.Vector Int -> A.Vector Visibility -> IO (A.Matrix Visibility)
convgrid2IO h@(GridHip c) gcf a p wbin v = do
  (out, hgt, wid) <- copyGrid a
  let A.Z A.:. w A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape gcf
      A.Z A.:. n = A.arrayShape v
  withForeignPtr out $ \o -> withCplx gcf $ \k -> withUVW p $ \pu pv _ -> withI wbin $ \wb -> withCplx v $ \vs ->
    c_convgrid2 c (fi hgt) (fi wid) o (fi n) (fi w) (fi q) (fi gh) (fi gw) k pu pv 1 wb vs >>= check h
  return (adoptGrid out hgt wid)

-- | degrid2 gcf a p wbin: the gather with convgrid2's coordinates (north star "degrid"; the reference has none)
degrid2IO :: GridHip -> A.Array A.DIM5 Visibility -> A.Matrix Visibility -> A.Vector BaseLines
          -> A.Vector Int -> IO (A.Vector Visibility)
degrid2IO h@(GridHip c) gcf a p wbin = do
  let A.Z A.:. w A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape gcf
      A.Z A.:. hgt A.:. wid = A.arrayShape a
      A.Z A.:. n = A.arrayShape wbin
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  withForeignPtr out $ \o -> withCplx gcf $ \k -> withCplx a $ \g -> withUVW p $ \pu pv _ -> withI wbin $ \wb ->
    c_degrid2 c (fi hgt) (fi wid) g (fi n) (fi w) (fi q) (fi gh) (fi gw) k pu pv 1 wb o >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out))

-- | convgrid3 / convgrid4 wkerns akerns a p index v  (src/Gridding.hs:246-252, 318-324: both produce this grid);
-- wkerns [W,Q,Q,S,S], akerns [A,S,S], index = (wbin, a1, a2)
awgridIO :: GridHip -> A.Array A.DIM5 Visibility -> A.Array A.DIM3 Visibility -> A.Matrix Visibility
         -> A.Vector BaseLines -> A.Vector (Int, Int, Int) -> A.Vector Visibility -> IO (A.Matrix Visibility)
awgridIO h@(GridHip c) wkerns akerns a p index v = do
  (out, hgt, wid) <- copyGrid a
  let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
      A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      A.Z A.:. n = A.arrayShape v
  withForeignPtr out $ \o -> withCplx wkerns $ \wk -> withCplx akerns $ \ak -> withUVW p $ \pu pv _ ->
    withIdx3 index $ \wb a1 a2 -> withCplx v $ \vs ->
      c_awgrid c (fi hgt) (fi wid) o (fi n) (fi w) (fi q) (fi s) (fi na) wk ak pu pv 1 wb a1 a2 vs >>= check h
  return (adoptGrid out hgt wid)

-- | the gather twin of convgrid4: wkerns akerns a p index -> one prediction per baseline, with the kernel awgridIO
-- scatters (conj . aw_kernel_fn2, not conjugated again); out-of-range indices predict 0 (the reference has no degrid)
awdegridIO :: GridHip -> A.Array A.DIM5 Visibility -> A.Array A.DIM3 Visibility -> A.Matrix Visibility
           -> A.Vector BaseLines -> A.Vector (Int, Int, Int) -> IO (A.Vector Visibility)
awdegridIO h@(GridHip c) wkerns akerns a p index = do
  let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
      A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      A.Z A.:. hgt A.:. wid = A.arrayShape a
      A.Z A.:. n = A.arrayShape index
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  withForeignPtr out $ \o -> withCplx wkerns $ \wk -> withCplx akerns $ \ak -> withCplx a $ \g ->
    withUVW p $ \pu pv _ -> withIdx3 index $ \wb a1 a2 ->
      c_awdegrid c (fi hgt) (fi wid) g (fi n) (fi w) (fi q) (fi s) (fi na) wk ak pu pv 1 wb a1 a2 o >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out))

-- ---------------------------------------------------------------------------------------------------------
-- ImagingFunctions (src/Gridding.hs:76-81): theta lam uvw src vis -> grid.  uvw in wavelengths; `src` is only used
-- by the aw variants (:475), which take the antenna vectors directly here.

imageSize :: F -> Int -> IO Int
imageSize theta lam = fi <$> c_image_size (realToFrac theta) (fi lam)

-- | simple_imaging  (src/Gridding.hs:84-93)
simpleImagingIO :: GridHip -> F -> Int -> A.Vector BaseLines -> A.Vector Visibility -> IO (A.Matrix Visibility)
simpleImagingIO h@(GridHip c) theta lam uvw vis = do
  n' <- imageSize theta lam
  out <- newGrid n'
  let A.Z A.:. n = A.arrayShape vis
  withForeignPtr out $ \o -> withUVW uvw $ \u v _ -> withCplx vis $ \vs ->
    c_simple_imaging c (realToFrac theta) (fi lam) (fi n) u v 1 vs o >>= check h
  return (adoptGrid out n' n')

-- | conv_imaging kv  (src/Gridding.hs:115-124)
convImagingIO :: GridHip -> A.Array A.DIM4 Visibility -> F -> Int -> A.Vector BaseLines -> A.Vector Visibility
              -> IO (A.Matrix Visibility)
convImagingIO h@(GridHip c) kv theta lam uvw vis = do
  n' <- imageSize theta lam
  out <- newGrid n'
  let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape kv
      A.Z A.:. n = A.arrayShape vis
  withForeignPtr out $ \o -> withCplx kv $ \k -> withUVW uvw $ \u v _ -> withCplx vis $ \vs ->
    c_conv_imaging c (fi q) (fi gh) (fi gw) k (realToFrac theta) (fi lam) (fi n) u v 1 vs o >>= check h
  return (adoptGrid out n' n')

-- | w_cache_imaging kernops otargs  (src/Gridding.hs:399-449): wstep, qpx, npixFF, npixKern of KernelOptions (:30-38)
wCacheImagingIO :: GridHip -> Int -> Int -> Int -> Int -> F -> Int -> A.Vector BaseLines -> A.Vector Visibility
                -> IO (A.Matrix Visibility)
wCacheImagingIO h@(GridHip c) wstep qpx npixFF npixKern theta lam uvw vis = do
  n' <- imageSize theta lam
  out <- newGrid n'
  let A.Z A.:. n = A.arrayShape vis
  withForeignPtr out $ \o -> withUVW uvw $ \u v w -> withCplx vis $ \vs ->
    c_w_cache_imaging c (fi wstep) (fi qpx) (fi npixFF) (fi npixKern) (realToFrac theta) (fi lam) (fi n) u v w 1 vs o
      >>= check h
  return (adoptGrid out n' n')

-- | aw_imaging / aw_imagingOld  (src/Gridding.hs:452-506); wvals = the W plane w-values findClosest searches
awImagingIO :: GridHip -> F -> Int -> A.Array A.DIM5 Visibility -> A.Vector BaseLine -> A.Array A.DIM3 Visibility
            -> A.Vector BaseLines -> A.Vector Antenna -> A.Vector Antenna -> A.Vector Visibility
            -> IO (A.Matrix Visibility)
awImagingIO h@(GridHip c) theta lam wkerns wvals akerns uvw ant1 ant2 vis = do
  n' <- imageSize theta lam
  out <- newGrid n'
  let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
      A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      A.Z A.:. n = A.arrayShape vis
  withForeignPtr out $ \o -> withCplx wkerns $ \wk -> withF wvals $ \wv -> withCplx akerns $ \ak ->
    withUVW uvw $ \u v ww -> withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withCplx vis $ \vs ->
      c_aw_imaging c (realToFrac theta) (fi lam) (fi w) (fi q) (fi s) (fi na) wk wv ak (fi n) u v ww 1 a1 a2 vs o
        >>= check h
  return (adoptGrid out n' n')

-- | which ImagingFunction do_imaging runs (the `imgfn` argument of src/Gridding.hs:509-519)
data ImagingKind
  = SimpleImaging                              -- ^ simple_imaging
  | ConvImaging (A.Array A.DIM4 Visibility)    -- ^ conv_imaging kv
  | WCacheImaging Int Int Int Int              -- ^ w_cache_imaging: wstep qpx npixFF npixKern
  | AwImaging (A.Array A.DIM5 Visibility) (A.Vector BaseLine) (A.Array A.DIM3 Visibility)
              (A.Vector Antenna) (A.Vector Antenna)
                                               -- ^ aw_imaging: wkerns wvals akerns ant1 ant2 (the `src` it reads)

-- | do_imaging theta lam uvw a1 a2 t f vis imgfn  (src/Gridding.hs:509-549): (image, psf, pmax).
-- uvw is the (n,3) row-major Matrix BaseLine as it comes from HDF5 (src/ImageDataset.hs:94-97): passed with
-- uv_stride = 3, the columns are sliced on the device (:524-526).  t, f are unused by these imaging functions; a1, a2
-- travel inside AwImaging (gridhip_do_imaging_aw: the image and PSF passes share each batch's kernel table).
doImagingIO :: GridHip -> F -> Int -> A.Matrix BaseLine -> A.Vector Visibility -> ImagingKind
            -> IO (A.Matrix F, A.Matrix F, F)
doImagingIO h@(GridHip c) theta lam uvw vis kind = do
  n' <- imageSize theta lam
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  psf <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let A.Z A.:. n = A.arrayShape vis
      run k wstep q npixFF gh gw kv =
        withForeignPtr img $ \pi' -> withForeignPtr psf $ \pp -> withF uvw $ \m -> withCplx vis $ \vs ->
          alloca $ \pm -> do
            c_do_imaging c k (fi wstep) (fi q) (fi npixFF) (fi gh) (fi gw) kv (realToFrac theta) (fi lam) (fi n)
                         m (m `advancePtr` 1) (m `advancePtr` 2) 3 vs pi' pp pm >>= check h
            realToFrac <$> peek pm
  pmax <- case kind of
    SimpleImaging -> run 0 (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) nullPtr
    ConvImaging kv ->
      let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape kv
      in withCplx kv $ \k -> run 1 (0 :: Int) q (0 :: Int) gh gw k
    WCacheImaging wstep q npixFF s -> run 2 wstep q npixFF s s nullPtr
    AwImaging wkerns wvals akerns ant1 ant2 ->
      let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
          A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      in withForeignPtr img $ \pi' -> withForeignPtr psf $ \pp -> withF uvw $ \m -> withCplx vis $ \vs ->
           withCplx wkerns $ \wk -> withF wvals $ \wv -> withCplx akerns $ \ak -> withI64 ant1 $ \a1 ->
             withI64 ant2 $ \a2 -> alloca $ \pm -> do
               c_do_imaging_aw c (realToFrac theta) (fi lam) (fi w) (fi q) (fi s) (fi na) wk wv ak (fi n)
                               m (m `advancePtr` 1) (m `advancePtr` 2) 3 a1 a2 vs pi' pp pm >>= check h
               realToFrac <$> peek pm
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr img), A.fromForeignPtrs sh (castForeignPtr psf), pmax)

-- | predict theta lam uvw model kind vis_sub: the visibilities of a real N x N model image (N = round (theta * lam)),
-- the exact adjoint of the imaging function `kind` applied to the centred forward transform of the model
-- (include/gridhip.h, gridhip_predict / gridhip_predict_aw); with Just vis_sub, vis_sub minus that (the residual of a
-- major cycle: doImagingIO -> model -> predictIO (Just vis) -> residual).  uvw as doImagingIO takes it (the (n,3)
-- Matrix BaseLine in wavelengths, uv_stride 3), not mirrored.
predictIO :: GridHip -> F -> Int -> A.Matrix BaseLine -> A.Matrix F -> ImagingKind -> Maybe (A.Vector Visibility)
          -> IO (A.Vector Visibility)
predictIO h@(GridHip c) theta lam uvw model kind visSub = do
  let A.Z A.:. n A.:. _ = A.arrayShape uvw
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  let withSub k = maybe (k nullPtr) (\s -> withCplx s k) visSub
      run k wstep q npixFF gh gw kv =
        withForeignPtr out $ \o -> withF uvw $ \m -> withF model $ \md -> withSub $ \sb ->
          c_predict c k (fi wstep) (fi q) (fi npixFF) (fi gh) (fi gw) kv (realToFrac theta) (fi lam) md (fi n)
                    m (m `advancePtr` 1) (m `advancePtr` 2) 3 sb o >>= check h
  case kind of
    SimpleImaging -> run 0 (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) nullPtr
    ConvImaging kv ->
      let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape kv
      in withCplx kv $ \k -> run 1 (0 :: Int) q (0 :: Int) gh gw k
    WCacheImaging wstep q npixFF s -> run 2 wstep q npixFF s s nullPtr
    AwImaging wkerns wvals akerns ant1 ant2 ->
      let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
          A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      in withForeignPtr out $ \o -> withF uvw $ \m -> withF model $ \md -> withSub $ \sb ->
           withCplx wkerns $ \wk -> withF wvals $ \wv -> withCplx akerns $ \ak -> withI64 ant1 $ \a1 ->
             withI64 ant2 $ \a2 ->
               c_predict_aw c (realToFrac theta) (fi lam) (fi w) (fi q) (fi s) (fi na) wk wv ak md (fi n)
                            m (m `advancePtr` 1) (m `advancePtr` 2) 3 a1 a2 sb o >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out))

-- | aw_gridding after its HDF5 reads (src/ImageDataset.hs:54-77) as one library call: uvw is /vis/uvw in METRES,
-- the (n,3) Matrix BaseLine, and f the frequency in Hz; uvw_lambda, doweight (on the UN-mirrored uvw, :59),
-- mirror_uvw, aw_imaging of vis1 * wt, make_grid_hermitian and real . ifft run on the device.  Returns the image
-- (not normalised, as in the reference) and its maximum, the `max` the reference's driver returns.
awGriddingIO :: GridHip -> F -> Int -> F -> A.Array A.DIM5 Visibility -> A.Vector BaseLine
             -> A.Array A.DIM3 Visibility -> A.Matrix BaseLine -> A.Vector Antenna -> A.Vector Antenna
             -> A.Vector Visibility -> IO (A.Matrix F, F)
awGriddingIO h@(GridHip c) theta lam f wkerns wvals akerns uvw ant1 ant2 vis = do
  n' <- imageSize theta lam
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
      A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
      A.Z A.:. n = A.arrayShape vis
  mx <- withForeignPtr img $ \pi' -> withF uvw $ \m -> withCplx vis $ \vs -> withCplx wkerns $ \wk ->
          withF wvals $ \wv -> withCplx akerns $ \ak -> withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 ->
            alloca $ \pm -> do
              c_aw_gridding c (realToFrac theta) (fi lam) (realToFrac f) (fi w) (fi q) (fi s) (fi na) wk wv ak (fi n)
                            m (m `advancePtr` 1) (m `advancePtr` 2) 3 a1 a2 vs pi' pm >>= check h
              realToFrac <$> peek pm
  return (A.fromForeignPtrs (A.Z A.:. n' A.:. n') (castForeignPtr img), mx)

-- ---------------------------------------------------------------------------------------------------------
-- Imagers (include/gridhip.h, gridhip_imager_*): device pointers only, like the plans, so the host arrays are staged
-- through gridhip_malloc / gridhip_memcpy_h2d here.

-- | an imager, its context, the visibilities it was created for and its image size
data ImagerH = ImagerH GridHip (Ptr Imager) Int Int

-- a device copy of `bytes` bytes at `src` for the duration of `k`
withDev :: GridHip -> Ptr a -> Int -> (Ptr b -> IO c) -> IO c
withDev h@(GridHip c) src bytes k = bracket open (\d -> () <$ c_free c d) $ \d -> do
  c_memcpy_h2d c d (castPtr src) (fi bytes) >>= check h
  k (castPtr d)
  where open = alloca $ \pp -> c_malloc c pp (fi (max 16 bytes)) >>= check h >> peek pp

-- | withImager h theta lam uvw kind k: bind the baselines `uvw` (the (n,3) Matrix BaseLine in wavelengths, not
-- mirrored, as doImagingIO and predictIO take it) and the imaging function `kind` once - mirror, weights, w-bins, kernel
-- tables, both binnings, the PSF - and run `k` with the imager; the loop of a major cycle is then imagerCycleIO alone.
withImager :: GridHip -> F -> Int -> A.Matrix BaseLine -> ImagingKind -> (ImagerH -> IO a) -> IO a
withImager h@(GridHip c) theta lam uvw kind k = do
  n' <- imageSize theta lam
  let A.Z A.:. n A.:. _ = A.arrayShape uvw
      make f = alloca $ \pp -> f pp >>= check h >> peek pp
      plain kd wstep q npixFF gh gw kv = withF uvw $ \m -> withDev h m (24 * n) $ \d ->
        make $ c_imager_create_dev c kd (fi wstep) (fi q) (fi npixFF) (fi gh) (fi gw) kv (realToFrac theta) (fi lam)
                                   (fi n) d (d `advancePtr` 1) (d `advancePtr` 2) 3
      open = case kind of
        SimpleImaging -> plain 0 (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) nullPtr
        ConvImaging kv ->
          let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape kv
          in withCplx kv $ \kp -> withDev h kp (16 * q * q * gh * gw) $ \dk -> plain 1 (0 :: Int) q (0 :: Int) gh gw dk
        WCacheImaging wstep q npixFF s -> plain 2 wstep q npixFF s s nullPtr
        AwImaging wkerns wvals akerns ant1 ant2 ->
          let A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
              A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
          in withF uvw $ \m -> withDev h m (24 * n) $ \d -> withCplx wkerns $ \wk ->
               withDev h wk (16 * w * q * q * s * s) $ \dwk -> withF wvals $ \wv -> withDev h wv (8 * w) $ \dwv ->
                 withCplx akerns $ \ak -> withDev h ak (16 * na * s * s) $ \dak -> withI64 ant1 $ \a1 ->
                   withDev h a1 (8 * n) $ \d1 -> withI64 ant2 $ \a2 -> withDev h a2 (8 * n) $ \d2 ->
                     make $ c_imager_create_aw_dev c (realToFrac theta) (fi lam) (fi w) (fi q) (fi s) (fi na) dwk dwv dak
                                                   (fi n) d (d `advancePtr` 1) (d `advancePtr` 2) 3 d1 d2
  bracket open (\p -> () <$ c_imager_destroy p) $ \p -> k (ImagerH h p n n')

-- | imagerCycleIO im model vis: the image of doImagingIO (predictIO (Just vis) model) for the imager's baselines
-- (of doImagingIO vis with Nothing), and the residual visibilities vis - predict model.
imagerCycleIO :: ImagerH -> Maybe (A.Matrix F) -> A.Vector Visibility -> IO (A.Matrix F, A.Vector Visibility)
imagerCycleIO (ImagerH h@(GridHip c) p n n') model vis = do
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  res <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  let withModel k = maybe (k nullPtr) (\m -> withF m $ \mp -> withDev h mp (8 * n' * n') k) model
  withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withModel $ \dm ->
    withForeignPtr img $ \pi' -> withDev h pi' (8 * n' * n') $ \di -> withForeignPtr res $ \pr -> do
      c_imager_cycle_dev p dm dv di dv >>= check h   -- (the residual in place, in the device copy of vis)
      c_memcpy_d2h c (castPtr pi') (castPtr di) (fi (8 * n' * n')) >>= check h
      c_memcpy_d2h c (castPtr pr) (castPtr dv) (fi (16 * n)) >>= check h
      c_synchronize c >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n' A.:. n') (castForeignPtr img), A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr res))

-- ---------------------------------------------------------------------------------------------------------
-- Deconvolution (include/gridhip.h, "deconvolution"): Hogbom CLEAN of a real N x N image.

-- | gain, threshold, niter, border, patch as gridhip_clean takes them
data CleanOptions = CleanOptions { cleanGain :: F, cleanThreshold :: F, cleanNiter :: Int, cleanBorder :: Int
                                 , cleanPatch :: Int }

-- [iterations, final peak, its flat index, flux added] per row of a stats block
statsRows :: Int -> Ptr CDouble -> IO [[F]]
statsRows rows p = mapM (\r -> map realToFrac <$> peekArray 4 (p `advancePtr` (4 * r))) [0 .. rows - 1]

-- | cleanIO h opts image psf model: (model + the components found, the residual, the stats) - the host form, synchronous
cleanIO :: GridHip -> CleanOptions -> A.Matrix F -> A.Matrix F -> A.Matrix F -> IO (A.Matrix F, A.Matrix F, [F])
cleanIO h@(GridHip c) (CleanOptions g t ni b pa) image psf model = do
  let A.Z A.:. n' A.:. _ = A.arrayShape image
      copyOf m = do o <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
                    withF m $ \s -> withForeignPtr o $ \d -> copyArray d s (n' * n')
                    return o
  res <- copyOf image
  mdl <- copyOf model
  st <- withF psf $ \pp -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pm -> allocaArray 4 $ \ps -> do
          c_clean c (fi n') pp pr pm (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ps >>= check h
          head <$> statsRows 1 ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerCleanIO im opts image model: cleanIO with the imager's own PSF (gridhip_imager_clean_dev; the host arrays are
-- staged as imagerCycleIO stages them)
imagerCleanIO :: ImagerH -> CleanOptions -> A.Matrix F -> A.Matrix F -> IO (A.Matrix F, A.Matrix F, [F])
imagerCleanIO (ImagerH h@(GridHip c) p _ n') (CleanOptions g t ni b pa) image model = do
  res <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
  st <- withF image $ \pi' -> withDev h pi' bytes $ \di -> withF model $ \pm -> withDev h pm bytes $ \dm ->
          allocaArray 4 $ \ps -> withDev h ps 32 $ \ds -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pq -> do
            c_imager_clean_dev p di dm (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ds >>= check h
            c_memcpy_d2h c (castPtr pr) (castPtr di) (fi bytes) >>= check h
            c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
            c_memcpy_d2h c (castPtr ps) (castPtr ds) 32 >>= check h
            c_synchronize c >>= check h
            head <$> statsRows 1 ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerDeconvolveIO im opts nmajor vis model: nmajor times (imagerCycleIO, imagerCleanIO) and one closing cycle in
-- one call on the device (gridhip_imager_deconvolve_dev): (the model, the closing residual image, one stats row per
-- major cycle)
imagerDeconvolveIO :: ImagerH -> CleanOptions -> Int -> A.Vector Visibility -> A.Matrix F
                   -> IO (A.Matrix F, A.Matrix F, [[F]])
imagerDeconvolveIO (ImagerH h@(GridHip c) p n n') (CleanOptions g t ni b pa) nmajor vis model = do
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
      rows = max 0 nmajor
  st <- withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withF model $ \pm -> withDev h pm bytes $ \dm ->
          withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> allocaArray (4 * rows) $ \ps ->
            withDev h ps (32 * rows) $ \ds -> withForeignPtr mdl $ \pq -> do
              c_imager_deconvolve_dev p dv dm di (fi nmajor) (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ds
                >>= check h
              c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr ps) (castPtr ds) (fi (32 * rows)) >>= check h
              c_synchronize c >>= check h
              statsRows rows ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr img), st)

-- ---------------------------------------------------------------------------------------------------------
-- Clean masks and noise-based stop levels (include/gridhip.h, "image statistics", "masks and noise-based stop levels").
-- A mask is one byte per cell, row-major, non-zero where a component may be centred.

-- | the clean mask (Nothing: none), nsigma and peak_frac of the stop level T = max(threshold, nsigma * sigma,
-- peak_frac * |first peak|)
data AutoOptions = AutoOptions { autoMask :: Maybe [Word8], autoNsigma :: F, autoPeakFrac :: F }

withMask :: Maybe [Word8] -> (Ptr Word8 -> IO a) -> IO a
withMask Nothing k = k nullPtr
withMask (Just m) k = withArray m k

-- | imageStatsIO h image mask border: [n, median, MAD, sigma = 1.4826 MAD, min, max, non-finite cells skipped, 0] of
-- the cells inside the border and the mask (gridhip_image_stats, the host form, synchronous)
imageStatsIO :: GridHip -> A.Matrix F -> Maybe [Word8] -> Int -> IO [F]
imageStatsIO h@(GridHip c) image mask border = do
  let A.Z A.:. n' A.:. _ = A.arrayShape image
  withF image $ \pi' -> withMask mask $ \pk -> allocaArray 8 $ \ps -> do
    c_image_stats c (fi n') pi' pk (fi border) ps >>= check h
    map realToFrac <$> peekArray 8 ps

-- | cleanAutoIO h opts auto sigma image psf model: cleanIO under a mask, stopping at T; sigma is the noise the nsigma
-- term multiplies (element 3 of imageStatsIO).  The stats are gridhip_clean's four, then [T, reason, first peak, 0].
cleanAutoIO :: GridHip -> CleanOptions -> AutoOptions -> F -> A.Matrix F -> A.Matrix F -> A.Matrix F
            -> IO (A.Matrix F, A.Matrix F, [F])
cleanAutoIO h@(GridHip c) (CleanOptions g t ni b pa) (AutoOptions mask ns pf) sigma image psf model = do
  let A.Z A.:. n' A.:. _ = A.arrayShape image
      copyOf m = do o <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
                    withF m $ \s -> withForeignPtr o $ \d -> copyArray d s (n' * n')
                    return o
  res <- copyOf image
  mdl <- copyOf model
  st <- withF psf $ \pp -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pm -> withMask mask $ \pk ->
          with (realToFrac sigma :: CDouble) $ \pn -> allocaArray 8 $ \ps -> do
            c_clean_auto c (fi n') pp pr pm (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) pk (realToFrac ns) pn
              (realToFrac pf) ps >>= check h
            map realToFrac <$> peekArray 8 ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerDeconvolveAutoIO im opts auto nmajor vis model: imagerDeconvolveIO whose minor cycles stop at nsigma times
-- the sigma of the map they clean (gridhip_imager_deconvolve_auto_dev): (the model, the closing residual image, one
-- row of 8 clean stats and one row of 8 image stats per major cycle)
imagerDeconvolveAutoIO :: ImagerH -> CleanOptions -> AutoOptions -> Int -> A.Vector Visibility -> A.Matrix F
                       -> IO (A.Matrix F, A.Matrix F, [[F]], [[F]])
imagerDeconvolveAutoIO (ImagerH h@(GridHip c) p n n') (CleanOptions g t ni b pa) (AutoOptions mask ns pf) nmajor vis model = do
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
      rows = max 0 nmajor
      rows8 q = mapM (\r -> map realToFrac <$> peekArray 8 (q `advancePtr` (8 * r))) [0 .. rows - 1]
      withDevMask Nothing k = k nullPtr
      withDevMask (Just m) k = withArray m $ \pk -> withDev h pk (n' * n') k
  withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withF model $ \pm -> withDev h pm bytes $ \dm ->
    withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> allocaArray (8 * rows) $ \ps ->
      withDev h ps (64 * rows) $ \ds -> allocaArray (8 * rows) $ \pis -> withDev h pis (64 * rows) $ \dis ->
        withDevMask mask $ \dk -> withForeignPtr mdl $ \pq -> do
          c_imager_deconvolve_auto_dev p dv dm di (fi nmajor) (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) dk
            (realToFrac ns) (realToFrac pf) ds dis >>= check h
          c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
          c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
          c_memcpy_d2h c (castPtr ps) (castPtr ds) (fi (64 * rows)) >>= check h
          c_memcpy_d2h c (castPtr pis) (castPtr dis) (fi (64 * rows)) >>= check h
          c_synchronize c >>= check h
          st <- rows8 ps
          ist <- rows8 pis
          let sh = A.Z A.:. n' A.:. n'
          return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr img), st, ist)

-- ---------------------------------------------------------------------------------------------------------
-- Auto-masking (include/gridhip.h, "auto-masking"): two levels, islands above the higher one pruned by size, kept with
-- the whole island above the lower level they lie in, grown, and OR-ed into the mask.

-- | absolute, (thr_hi, thr_lo), (nsigma_hi, nsigma_lo), peak_frac, min_cells, grow of gridhip_automask
data AutomaskOptions = AutomaskOptions { amAbsolute :: Bool, amThr :: (F, F), amNsigma :: (F, F), amPeakFrac :: F
                                       , amMinCells :: Int, amGrow :: Int }

-- | automaskIO h opts sigma border image mask: (the updated mask, [T_hi, T_lo, P, components of H, surviving the prune,
-- components of L kept, cells newly set, reason]); sigma is the noise the nsigma terms multiply (element 3 of
-- imageStatsIO) - gridhip_automask, the host form, synchronous
automaskIO :: GridHip -> AutomaskOptions -> F -> Int -> A.Matrix F -> [Word8] -> IO ([Word8], [F])
automaskIO h@(GridHip c) (AutomaskOptions ab (th, tl) (nh, nl) pf mc gr) sigma border image mask = do
  let A.Z A.:. n' A.:. _ = A.arrayShape image
  withF image $ \pi' -> withArray mask $ \pk -> with (realToFrac sigma :: CDouble) $ \pn -> allocaArray 8 $ \ps -> do
    c_automask c (fi n') pi' pk (fi border) (if ab then 1 else 0) (realToFrac th) (realToFrac tl) (realToFrac nh)
      (realToFrac nl) pn (realToFrac pf) (fi mc) (fi gr) ps >>= check h
    m <- peekArray (n' * n') pk
    st <- map realToFrac <$> peekArray 8 ps
    return (m, st)

-- | imagerDeconvolveAutomaskIO im opts auto am nmajor vis model: imagerDeconvolveAutoIO whose mask every major cycle
-- extends from the map it is about to clean (gridhip_imager_deconvolve_automask_dev); autoMask is the starting mask
-- (Nothing: zeros).  Returns (the model, the closing residual image, the accumulated mask, and per major cycle one row of
-- 8 clean stats, one of 8 image stats and one of 8 automask stats)
imagerDeconvolveAutomaskIO :: ImagerH -> CleanOptions -> AutoOptions -> AutomaskOptions -> Int -> A.Vector Visibility
                           -> A.Matrix F -> IO (A.Matrix F, A.Matrix F, [Word8], [[F]], [[F]], [[F]])
imagerDeconvolveAutomaskIO (ImagerH h@(GridHip c) p n n') (CleanOptions g t ni b pa) (AutoOptions mask ns pf)
                           (AutomaskOptions ab (th, tl) (nh, nl) apf mc gr) nmajor vis model = do
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
      rows = max 0 nmajor
      rows8 q = mapM (\r -> map realToFrac <$> peekArray 8 (q `advancePtr` (8 * r))) [0 .. rows - 1]
      start = maybe (replicate (n' * n') 0) id mask
  withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withF model $ \pm -> withDev h pm bytes $ \dm ->
    withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> allocaArray (8 * rows) $ \ps ->
      withDev h ps (64 * rows) $ \ds -> allocaArray (8 * rows) $ \pis -> withDev h pis (64 * rows) $ \dis ->
        allocaArray (8 * rows) $ \pas -> withDev h pas (64 * rows) $ \das ->
          withArray start $ \pk -> withDev h pk (n' * n') $ \dk -> withForeignPtr mdl $ \pq -> do
            c_imager_deconvolve_automask_dev p dv dm di (fi nmajor) (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) dk
              (realToFrac ns) (realToFrac pf) (if ab then 1 else 0) (realToFrac th) (realToFrac tl) (realToFrac nh)
              (realToFrac nl) (realToFrac apf) (fi mc) (fi gr) ds dis das >>= check h
            c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
            c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
            c_memcpy_d2h c (castPtr pk) (castPtr dk) (fi (n' * n')) >>= check h
            c_memcpy_d2h c (castPtr ps) (castPtr ds) (fi (64 * rows)) >>= check h
            c_memcpy_d2h c (castPtr pis) (castPtr dis) (fi (64 * rows)) >>= check h
            c_memcpy_d2h c (castPtr pas) (castPtr das) (fi (64 * rows)) >>= check h
            c_synchronize c >>= check h
            st <- rows8 ps
            ist <- rows8 pis
            ast <- rows8 pas
            m <- peekArray (n' * n') pk
            let sh = A.Z A.:. n' A.:. n'
            return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr img), m, st, ist, ast)

-- ---------------------------------------------------------------------------------------------------------
-- Multi-scale deconvolution (include/gridhip.h, "multi-scale deconvolution"): scales in cells increasing from 0, one
-- bias per scale; both are host arrays for every form.  A stats row is [iterations, final peak, its flat index, the
-- last component's scale, flux added, 0, components per scale x 6].

msStatsRows :: Int -> Ptr CDouble -> IO [[F]]
msStatsRows rows p = mapM (\r -> map realToFrac <$> peekArray 12 (p `advancePtr` (12 * r))) [0 .. rows - 1]

-- the default bias of a scale list: 1 - 0.6 a_s / a_max
msDefaultBias :: [F] -> [F]
msDefaultBias scales = let amax = maximum scales in [if amax > 0 then 1 - 0.6 * a / amax else 1 | a <- scales]

-- | mscleanIO h opts scales bias image psf model: cleanIO with multi-scale components - the host form, synchronous
mscleanIO :: GridHip -> CleanOptions -> [F] -> [F] -> A.Matrix F -> A.Matrix F -> A.Matrix F
          -> IO (A.Matrix F, A.Matrix F, [F])
mscleanIO h@(GridHip c) (CleanOptions g t ni b pa) scales bias image psf model = do
  let A.Z A.:. n' A.:. _ = A.arrayShape image
      copyOf m = do o <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
                    withF m $ \s -> withForeignPtr o $ \d -> copyArray d s (n' * n')
                    return o
  res <- copyOf image
  mdl <- copyOf model
  st <- withF psf $ \pp -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pm -> allocaArray 12 $ \ps ->
          withArray (map realToFrac scales) $ \psc -> withArray (map realToFrac bias) $ \pbi -> do
            c_msclean c (fi n') pp pr pm (fi (length scales)) psc pbi (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ps
              >>= check h
            head <$> msStatsRows 1 ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerMscleanIO im opts scales bias image model: mscleanIO with the imager's own PSF (gridhip_imager_msclean_dev);
-- the imager keeps the cross-PSFs of the scale list between calls
imagerMscleanIO :: ImagerH -> CleanOptions -> [F] -> [F] -> A.Matrix F -> A.Matrix F -> IO (A.Matrix F, A.Matrix F, [F])
imagerMscleanIO (ImagerH h@(GridHip c) p _ n') (CleanOptions g t ni b pa) scales bias image model = do
  res <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
  st <- withF image $ \pi' -> withDev h pi' bytes $ \di -> withF model $ \pm -> withDev h pm bytes $ \dm ->
          allocaArray 12 $ \ps -> withDev h ps 96 $ \ds -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pq ->
            withArray (map realToFrac scales) $ \psc -> withArray (map realToFrac bias) $ \pbi -> do
              c_imager_msclean_dev p di dm (fi (length scales)) psc pbi (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ds
                >>= check h
              c_memcpy_d2h c (castPtr pr) (castPtr di) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr ps) (castPtr ds) 96 >>= check h
              c_synchronize c >>= check h
              head <$> msStatsRows 1 ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerMsDeconvolveIO im opts scales bias nmajor vis model: imagerDeconvolveIO with the multi-scale minor cycle
-- (gridhip_imager_msdeconvolve_dev): (the model, the closing residual image, one stats row per major cycle)
imagerMsDeconvolveIO :: ImagerH -> CleanOptions -> [F] -> [F] -> Int -> A.Vector Visibility -> A.Matrix F
                     -> IO (A.Matrix F, A.Matrix F, [[F]])
imagerMsDeconvolveIO (ImagerH h@(GridHip c) p n n') (CleanOptions g t ni b pa) scales bias nmajor vis model = do
  img <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
      rows = max 0 nmajor
  st <- withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withF model $ \pm -> withDev h pm bytes $ \dm ->
          withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> allocaArray (12 * rows) $ \ps ->
            withDev h ps (96 * rows) $ \ds -> withForeignPtr mdl $ \pq ->
              withArray (map realToFrac scales) $ \psc -> withArray (map realToFrac bias) $ \pbi -> do
                c_imager_msdeconvolve_dev p dv dm di (fi nmajor) (fi (length scales)) psc pbi (realToFrac g) (realToFrac t)
                  (fi ni) (fi b) (fi pa) ds >>= check h
                c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
                c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
                c_memcpy_d2h c (castPtr ps) (castPtr ds) (fi (96 * rows)) >>= check h
                c_synchronize c >>= check h
                msStatsRows rows ps
  let sh = A.Z A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr img), st)

-- ---------------------------------------------------------------------------------------------------------
-- Joint deconvolution (include/gridhip.h, "joint deconvolution"): P images of one sky, as [P][N][N] arrays.

-- | the statistic the joint search maximises: the weighted sum of the planes, or of their squares
data JointMetric = JointSum | JointSumSq deriving (Eq, Show)

-- | jcleanIO h opts auto sigma metric weights images psfs models: the joint CLEAN of the P residual images with one PSF
-- ([1][N][N]) or one per plane ([P][N][N]); weights Nothing is 1 for every plane; mask, nsigma, sigma and peak_frac as for
-- cleanAutoIO.  (models + the components found, the residuals, the 16 stats [iterations, s at the final peak, its flat
-- index, L, reason, first s, 0, 0, flux_0 .. flux_7]) - the host form, synchronous
jcleanIO :: GridHip -> CleanOptions -> AutoOptions -> F -> JointMetric -> Maybe [F] -> A.Array A.DIM3 F
         -> A.Array A.DIM3 F -> A.Array A.DIM3 F -> IO (A.Array A.DIM3 F, A.Array A.DIM3 F, [F])
jcleanIO h@(GridHip c) (CleanOptions g t ni b pa) (AutoOptions mask ns pf) sigma metric weights images psfs models = do
  let A.Z A.:. np A.:. n' A.:. _ = A.arrayShape images
      A.Z A.:. nq A.:. _ A.:. _ = A.arrayShape psfs
      copyOf m = do o <- mallocForeignPtrArray (np * n' * n') :: IO (ForeignPtr CDouble)
                    withF m $ \s -> withForeignPtr o $ \d -> copyArray d s (np * n' * n')
                    return o
      withWeights Nothing k = k nullPtr
      withWeights (Just w) k = withArray (map realToFrac w) k
  res <- copyOf images
  mdl <- copyOf models
  st <- withF psfs $ \pp -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pm -> withMask mask $ \pk ->
          withWeights weights $ \pw -> with (realToFrac sigma :: CDouble) $ \pn -> allocaArray 16 $ \ps -> do
            c_jclean c (fi n') (fi np) (fi nq) pp pr pm pw (if metric == JointSum then 0 else 1) (realToFrac g)
              (realToFrac t) (fi ni) (fi b) (fi pa) pk (realToFrac ns) pn (realToFrac pf) ps >>= check h
            map realToFrac <$> peekArray 16 ps
  let sh = A.Z A.:. np A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- ---------------------------------------------------------------------------------------------------------
-- Wide-band imaging (include/gridhip.h, "wide-band imaging"): T Taylor terms of the sky, as [T][N][N] arrays.

-- [iterations, a_0 at the final peak, its flat index, flux_0 .. flux_3, reason] per row of a stats block
mfStatsRows :: Int -> Ptr CDouble -> IO [[F]]
mfStatsRows rows p = mapM (\r -> map realToFrac <$> peekArray 8 (p `advancePtr` (8 * r))) [0 .. rows - 1]

-- | mfcleanIO h opts images psfs models: the multi-term CLEAN of the T residual images with the 2T - 1 spectral PSFs:
-- (models + the components found, the residuals, the stats) - the host form, synchronous
mfcleanIO :: GridHip -> CleanOptions -> A.Array A.DIM3 F -> A.Array A.DIM3 F -> A.Array A.DIM3 F
          -> IO (A.Array A.DIM3 F, A.Array A.DIM3 F, [F])
mfcleanIO h@(GridHip c) (CleanOptions g t ni b pa) images psfs models = do
  let A.Z A.:. nt A.:. n' A.:. _ = A.arrayShape images
      copyOf m = do o <- mallocForeignPtrArray (nt * n' * n') :: IO (ForeignPtr CDouble)
                    withF m $ \s -> withForeignPtr o $ \d -> copyArray d s (nt * n' * n')
                    return o
  res <- copyOf images
  mdl <- copyOf models
  st <- withF psfs $ \pp -> withForeignPtr res $ \pr -> withForeignPtr mdl $ \pm -> allocaArray 8 $ \ps -> do
          c_mfclean c (fi n') (fi nt) pp pr pm (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ps >>= check h
          head <$> mfStatsRows 1 ps
  let sh = A.Z A.:. nt A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr res), st)

-- | imagerSetSpectralIO im nterms x: give the imager nterms Taylor terms, x_k = (nu_k - nu_0) / nu_0 per visibility
-- (gridhip_imager_set_spectral_dev: it builds and keeps the 2 nterms - 1 spectral PSFs)
imagerSetSpectralIO :: ImagerH -> Int -> A.Vector F -> IO ()
imagerSetSpectralIO (ImagerH h p n _) nterms x = withF x $ \px -> withDev h px (8 * n) $ \dx ->
  c_imager_set_spectral_dev p (fi nterms) dx >>= check h

-- | imagerMfsCycleIO im nterms models vis: one wide-band major-cycle step (gridhip_imager_mfs_cycle_dev) of an imager
-- that has had imagerSetSpectralIO with nterms: the nterms residual images of vis minus the prediction of the nterms
-- models (of vis with Nothing), and the residual visibilities
imagerMfsCycleIO :: ImagerH -> Int -> Maybe (A.Array A.DIM3 F) -> A.Vector Visibility
                 -> IO (A.Array A.DIM3 F, A.Vector Visibility)
imagerMfsCycleIO (ImagerH h@(GridHip c) p n n') nterms models vis = do
  let bytes = 8 * nterms * n' * n'
  img <- mallocForeignPtrArray (nterms * n' * n') :: IO (ForeignPtr CDouble)
  res <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  let withModels k = maybe (k nullPtr) (\m -> withF m $ \mp -> withDev h mp bytes k) models
  withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withModels $ \dm ->
    withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> withForeignPtr res $ \pr -> do
      c_imager_mfs_cycle_dev p dm dv di dv >>= check h   -- (the residual in place, in the device copy of vis)
      c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
      c_memcpy_d2h c (castPtr pr) (castPtr dv) (fi (16 * n)) >>= check h
      c_synchronize c >>= check h
  return ( A.fromForeignPtrs (A.Z A.:. nterms A.:. n' A.:. n') (castForeignPtr img)
         , A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr res) )

-- | imagerMfDeconvolveIO im opts nterms nmajor vis models: nmajor times (imagerMfsCycleIO, the multi-term CLEAN) and
-- one closing cycle in one call on the device (gridhip_imager_mfdeconvolve_dev): (the models, the closing residual
-- images, one row of 8 stats per major cycle)
imagerMfDeconvolveIO :: ImagerH -> CleanOptions -> Int -> Int -> A.Vector Visibility -> A.Array A.DIM3 F
                     -> IO (A.Array A.DIM3 F, A.Array A.DIM3 F, [[F]])
imagerMfDeconvolveIO (ImagerH h@(GridHip c) p n n') (CleanOptions g t ni b pa) nterms nmajor vis models = do
  img <- mallocForeignPtrArray (nterms * n' * n') :: IO (ForeignPtr CDouble)
  mdl <- mallocForeignPtrArray (nterms * n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * nterms * n' * n'
      rows = max 0 nmajor
  st <- withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withF models $ \pm -> withDev h pm bytes $ \dm ->
          withForeignPtr img $ \pi' -> withDev h pi' bytes $ \di -> allocaArray (8 * rows) $ \ps ->
            withDev h ps (64 * rows) $ \ds -> withForeignPtr mdl $ \pq -> do
              c_imager_mfdeconvolve_dev p dv dm di (fi nmajor) (realToFrac g) (realToFrac t) (fi ni) (fi b) (fi pa) ds
                >>= check h
              c_memcpy_d2h c (castPtr pi') (castPtr di) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr pq) (castPtr dm) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr ps) (castPtr ds) (fi (64 * rows)) >>= check h
              c_synchronize c >>= check h
              mfStatsRows rows ps
  let sh = A.Z A.:. nterms A.:. n' A.:. n'
  return (A.fromForeignPtrs sh (castForeignPtr mdl), A.fromForeignPtrs sh (castForeignPtr img), st)

-- ---------------------------------------------------------------------------------------------------------
-- Restoring beam and restore (include/gridhip.h, "restoring beam and restore").  A beam is the 8 values
-- [A, B, C, bmaj, bmin, bpa, ncells, ok] of the fit: FWHMs in cells, bpa in radians, ok = 0 and NaNs when it failed.

-- | fitBeamIO h window cut psf: the elliptical Gaussian fitted to the PSF's main lobe - the host form, synchronous
fitBeamIO :: GridHip -> Int -> F -> A.Matrix F -> IO [F]
fitBeamIO h@(GridHip c) window cut psf = do
  let A.Z A.:. n' A.:. _ = A.arrayShape psf
  withF psf $ \pp -> allocaArray 8 $ \pb -> do
    c_fit_beam c (fi n') pp (fi window) (realToFrac cut) pb >>= check h
    map realToFrac <$> peekArray 8 pb

-- | restoreIO h support beam model residual: model convolved with the beam over +-support cells (1 to 32) + residual,
-- in units per beam - the host form, synchronous; a failed beam is refused
restoreIO :: GridHip -> Int -> [F] -> A.Matrix F -> A.Matrix F -> IO (A.Matrix F)
restoreIO h@(GridHip c) support beam model residual = do
  let A.Z A.:. n' A.:. _ = A.arrayShape model
  out <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  withF model $ \pm -> withF residual $ \pr -> withArray (map realToFrac beam) $ \pb -> withForeignPtr out $ \po ->
    c_restore c (fi n') pm pr pb (fi support) po >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n' A.:. n') (castForeignPtr out))

-- | imagerBeamIO im window cut: fitBeamIO on the imager's own PSF (gridhip_imager_beam_dev)
imagerBeamIO :: ImagerH -> Int -> F -> IO [F]
imagerBeamIO (ImagerH h@(GridHip c) p _ _) window cut =
  allocaArray 8 $ \pb -> withDev h pb 64 $ \db -> do
    c_imager_beam_dev p (fi window) (realToFrac cut) db >>= check h
    c_memcpy_d2h c (castPtr pb) (castPtr db) 64 >>= check h
    c_synchronize c >>= check h
    map realToFrac <$> peekArray 8 pb

-- | imagerRestoreIO im window cut support model residual: (the restored image, the beam fitted to the imager's own
-- PSF) in one call on the device (gridhip_imager_restore_dev; the host arrays are staged as imagerCycleIO stages them).
-- A failed fit gives an image of NaNs and a beam whose ok is 0.
imagerRestoreIO :: ImagerH -> Int -> F -> Int -> A.Matrix F -> A.Matrix F -> IO (A.Matrix F, [F])
imagerRestoreIO (ImagerH h@(GridHip c) p _ n') window cut support model residual = do
  out <- mallocForeignPtrArray (n' * n') :: IO (ForeignPtr CDouble)
  let bytes = 8 * n' * n'
  beam <- withF model $ \pm -> withDev h pm bytes $ \dm -> withF residual $ \pr -> withDev h pr bytes $ \dr ->
            allocaArray 8 $ \pb -> withDev h pb 64 $ \db -> withForeignPtr out $ \po -> do
              c_imager_restore_dev p dm dr (fi window) (realToFrac cut) (fi support) dr db >>= check h
              c_memcpy_d2h c (castPtr po) (castPtr dr) (fi bytes) >>= check h
              c_memcpy_d2h c (castPtr pb) (castPtr db) 64 >>= check h
              c_synchronize c >>= check h
              map realToFrac <$> peekArray 8 pb
  return (A.fromForeignPtrs (A.Z A.:. n' A.:. n') (castForeignPtr out), beam)

-- ---------------------------------------------------------------------------------------------------------
-- Imaging weights (include/gridhip.h, "imaging weights").  stats are the 8 values
-- [sum w, sum w^2 / s, sum s, noise, f^2, n_used, n_flagged, n_outside].

data WeightMode = NaturalWeighting | UniformWeighting | BriggsWeighting

-- | the mode, Briggs' robust and the taper's sigma in wavelengths (0: no taper)
data Weighting = Weighting { weightMode :: WeightMode, weightRobust :: F, weightTaper :: F }

modeCode :: WeightMode -> CInt
modeCode NaturalWeighting = 0
modeCode UniformWeighting = 1
modeCode BriggsWeighting  = 2

-- | weightsIO h theta lam weighting uvw wt: the imaging weights of the baselines `uvw` (the (n,3) Matrix BaseLine in
-- wavelengths, taken as given) with the data weights `wt` (Nothing: ones; a value that is not > 0 flags its visibility)
-- and the stats - the host form, synchronous
weightsIO :: GridHip -> F -> Int -> Weighting -> A.Matrix BaseLine -> Maybe (A.Vector F) -> IO (A.Vector F, [F])
weightsIO h@(GridHip c) theta lam (Weighting m r t) uvw wt = do
  let A.Z A.:. n A.:. _ = A.arrayShape uvw
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray n :: IO (ForeignPtr CDouble)
  st <- withF uvw $ \p -> withWt $ \ps -> withForeignPtr out $ \po -> allocaArray 8 $ \pst -> do
          c_weights c (realToFrac theta) (fi lam) (fi n) p (p `advancePtr` 1) 3 ps (modeCode m) (realToFrac r)
                    (realToFrac t) po pst >>= check h
          map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out), st)

-- the data weights on the device for the duration of `k` (NULL for Nothing)
withDevWeights :: GridHip -> Int -> Maybe (A.Vector F) -> (Ptr CDouble -> IO a) -> IO a
withDevWeights h n wt k = maybe (k nullPtr) (\s -> withF s $ \ps -> withDev h ps (8 * n) k) wt

-- | imagerCreateWeightedIO h theta lam weighting wt uvw kind: withImager's creation for SimpleImaging, ConvImaging and
-- WCacheImaging with a weighting (gridhip_imager_create_weighted_dev); the density is taken on the mirrored baselines
-- and a flagged visibility contributes nothing to any image.  The caller ends with imagerDestroyIO.
imagerCreateWeightedIO :: GridHip -> F -> Int -> Weighting -> Maybe (A.Vector F) -> A.Matrix BaseLine -> ImagingKind
                       -> IO ImagerH
imagerCreateWeightedIO h@(GridHip c) theta lam (Weighting m r t) wt uvw kind = do
  n' <- imageSize theta lam
  let A.Z A.:. n A.:. _ = A.arrayShape uvw
      plain kd wstep q npixFF gh gw kv = withF uvw $ \mp -> withDev h mp (24 * n) $ \d -> withDevWeights h n wt $ \dw ->
        alloca $ \pp -> do
          c_imager_create_weighted_dev c kd (fi wstep) (fi q) (fi npixFF) (fi gh) (fi gw) kv (realToFrac theta) (fi lam)
                                       (fi n) d (d `advancePtr` 1) (d `advancePtr` 2) 3 (modeCode m) (realToFrac r)
                                       (realToFrac t) dw pp >>= check h
          peek pp
  p <- case kind of
    SimpleImaging -> plain 0 (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) (0 :: Int) nullPtr
    ConvImaging kv ->
      let A.Z A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape kv
      in withCplx kv $ \kp -> withDev h kp (16 * q * q * gh * gw) $ \dk -> plain 1 (0 :: Int) q (0 :: Int) gh gw dk
    WCacheImaging wstep q npixFF s -> plain 2 wstep q npixFF s s nullPtr
    AwImaging {} -> error "imagerCreateWeightedIO: AwImaging is imagerCreateAwWeightedIO's"
  return (ImagerH h p n n')

-- | imagerCreateAwWeightedIO h theta lam weighting wt uvw wkerns wvals akerns ant1 ant2: the same for aw_imaging
-- (gridhip_imager_create_aw_weighted_dev)
imagerCreateAwWeightedIO :: GridHip -> F -> Int -> Weighting -> Maybe (A.Vector F) -> A.Matrix BaseLine
                         -> A.Array A.DIM5 Visibility -> A.Vector BaseLine -> A.Array A.DIM3 Visibility
                         -> A.Vector Antenna -> A.Vector Antenna -> IO ImagerH
imagerCreateAwWeightedIO h@(GridHip c) theta lam (Weighting m r t) wt uvw wkerns wvals akerns ant1 ant2 = do
  n' <- imageSize theta lam
  let A.Z A.:. n A.:. _ = A.arrayShape uvw
      A.Z A.:. w A.:. q A.:. _ A.:. s A.:. _ = A.arrayShape wkerns
      A.Z A.:. na A.:. _ A.:. _ = A.arrayShape akerns
  p <- withF uvw $ \mp -> withDev h mp (24 * n) $ \d -> withCplx wkerns $ \wk ->
         withDev h wk (16 * w * q * q * s * s) $ \dwk -> withF wvals $ \wv -> withDev h wv (8 * w) $ \dwv ->
           withCplx akerns $ \ak -> withDev h ak (16 * na * s * s) $ \dak -> withI64 ant1 $ \a1 ->
             withDev h a1 (8 * n) $ \d1 -> withI64 ant2 $ \a2 -> withDev h a2 (8 * n) $ \d2 ->
               withDevWeights h n wt $ \dw -> alloca $ \pp -> do
                 c_imager_create_aw_weighted_dev c (realToFrac theta) (fi lam) (fi w) (fi q) (fi s) (fi na) dwk dwv dak
                                                 (fi n) d (d `advancePtr` 1) (d `advancePtr` 2) 3 d1 d2 (modeCode m)
                                                 (realToFrac r) (realToFrac t) dw pp >>= check h
                 peek pp
  return (ImagerH h p n n')

-- | release an imager made by imagerCreateWeightedIO / imagerCreateAwWeightedIO
imagerDestroyIO :: ImagerH -> IO ()
imagerDestroyIO (ImagerH _ p _ _) = () <$ c_imager_destroy p

-- | imagerWeightStatsIO im: the stats of the weighting the imager was created with (gridhip_imager_weight_stats_dev)
imagerWeightStatsIO :: ImagerH -> IO [F]
imagerWeightStatsIO (ImagerH h@(GridHip c) p _ _) =
  allocaArray 8 $ \ps -> withDev h ps 64 $ \ds -> do
    c_imager_weight_stats_dev p ds >>= check h
    c_memcpy_d2h c (castPtr ps) (castPtr ds) 64 >>= check h
    c_synchronize c >>= check h
    map realToFrac <$> peekArray 8 ps

-- ---------------------------------------------------------------------------------------------------------
-- Gain calibration (include/gridhip.h, "gain calibration"): per-antenna gains by StEFCal, their application, and the
-- selfcal step of an imager.

-- | how a solve runs: phase only or amplitude and phase; the reference antenna (Nothing: no rotation); the most
-- iterations and the relative change that stops them on the device (0: never early)
data GainSolve = GainSolve { gainPhaseOnly :: Bool, gainRefant :: Maybe Int, gainNiter :: Int, gainTol :: F }

solveCodes :: GainSolve -> (CInt, Int64, Int64, CDouble)
solveCodes (GainSolve po ref niter tol) = (if po then 1 else 0, maybe (-1) fi ref, fi niter, realToFrac tol)

-- | gaincalIO h solve nant nslots ant1 ant2 slot wt vis model: the [nslots][nant] gains of vis ~ g_p model conj(g_q)
-- starting from 1, and the 8 stats - the host form, synchronous.  slot Nothing: one interval; wt Nothing: ones.
gaincalIO :: GridHip -> GainSolve -> Int -> Int -> A.Vector Antenna -> A.Vector Antenna -> Maybe (A.Vector Antenna)
          -> Maybe (A.Vector F) -> A.Vector Visibility -> A.Vector Visibility -> IO (A.Matrix Visibility, [F])
gaincalIO h@(GridHip c) solve nant nslots ant1 ant2 slot wt vis model = do
  let A.Z A.:. n = A.arrayShape vis
      (mode, ref, niter, tol) = solveCodes solve
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray (2 * nslots * nant) :: IO (ForeignPtr CDouble)
  st <- withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withWt $ \ps -> withCplx vis $ \vs ->
          withCplx model $ \ms -> withForeignPtr out $ \po -> allocaArray 8 $ \pst -> do
            c_gaincal c (fi n) (fi nant) (fi nslots) a1 a2 sl vs ms ps mode ref 0 niter tol po pst >>= check h
            map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. nslots A.:. nant) (castForeignPtr out), st)

-- | applyGainsIO h inverse gains ant1 ant2 slot wt vis: (the visibilities, the weights) after the gains - True: data
-- corrected, vis / (g_p conj(g_q)) with weights |g_p|^2 |g_q|^2 wt and weight 0 where there is no usable gain; False: a
-- model corrupted, g_p vis conj(g_q) - the host form, synchronous
applyGainsIO :: GridHip -> Bool -> A.Matrix Visibility -> A.Vector Antenna -> A.Vector Antenna
             -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Vector Visibility
             -> IO (A.Vector Visibility, A.Vector F)
applyGainsIO h@(GridHip c) inverse gains ant1 ant2 slot wt vis = do
  let A.Z A.:. n = A.arrayShape vis
      A.Z A.:. nslots A.:. nant = A.arrayShape gains
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  wout <- mallocForeignPtrArray n :: IO (ForeignPtr CDouble)
  withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withWt $ \ps -> withCplx gains $ \g ->
    withCplx vis $ \vs -> withForeignPtr out $ \po -> withForeignPtr wout $ \pw ->
      c_apply_gains c (fi n) (fi nant) (fi nslots) a1 a2 sl g (if inverse then 1 else 0) vs ps po pw >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out), A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr wout))

-- | imagerSelfcalIO im solve nant nslots ant1 ant2 slot wt model vis: one self-calibration step
-- (gridhip_imager_selfcal_dev: predict, solve, correct as one chain on the device) -> (gains, the corrected
-- visibilities, their weights, the 8 stats)
imagerSelfcalIO :: ImagerH -> GainSolve -> Int -> Int -> A.Vector Antenna -> A.Vector Antenna
                -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Matrix F -> A.Vector Visibility
                -> IO (A.Matrix Visibility, A.Vector Visibility, A.Vector F, [F])
imagerSelfcalIO (ImagerH h@(GridHip c) p n n') solve nant nslots ant1 ant2 slot wt model vis = do
  let (mode, ref, niter, tol) = solveCodes solve
      cells = nslots * nant
      withSlot k = maybe (k nullPtr) (\s -> withI64 s $ \sp -> withDev h sp (8 * n) k) slot
  g <- mallocForeignPtrArray (2 * cells) :: IO (ForeignPtr CDouble)
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  wout <- mallocForeignPtrArray n :: IO (ForeignPtr CDouble)
  st <- withI64 ant1 $ \a1 -> withDev h a1 (8 * n) $ \d1 -> withI64 ant2 $ \a2 -> withDev h a2 (8 * n) $ \d2 ->
          withSlot $ \ds -> withDevWeights h n wt $ \dw -> withF model $ \mp -> withDev h mp (8 * n' * n') $ \dm ->
            withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withForeignPtr g $ \pg ->
              withDev h pg (16 * cells) $ \dg -> withForeignPtr wout $ \pw -> withDev h pw (8 * n) $ \dwo ->
                withForeignPtr out $ \po -> allocaArray 8 $ \pst -> withDev h pst 64 $ \dst -> do
                  -- (the corrected visibilities in place, in the device copy of vis)
                  c_imager_selfcal_dev p dm dv (fi nant) (fi nslots) d1 d2 ds dw mode ref 0 niter tol dg dv dwo dst
                    >>= check h
                  c_memcpy_d2h c (castPtr pg) (castPtr dg) (fi (16 * cells)) >>= check h
                  c_memcpy_d2h c (castPtr po) (castPtr dv) (fi (16 * n)) >>= check h
                  c_memcpy_d2h c (castPtr pw) (castPtr dwo) (fi (8 * n)) >>= check h
                  c_memcpy_d2h c (castPtr pst) (castPtr dst) 64 >>= check h
                  c_synchronize c >>= check h
                  map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. nslots A.:. nant) (castForeignPtr g), A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out),
          A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr wout), st)

-- ---------------------------------------------------------------------------------------------------------
-- Direction-dependent calibration (include/gridhip.h, "direction-dependent calibration"): D gain sets per antenna at
-- once, the subtraction of corrupted directions, and the peel step of an imager.

-- | ddcalIO h solve nant nslots ant1 ant2 slot wt vis models: the [D][nslots][nant] gains of
-- vis ~ sum_d g_dp models_d conj(g_dq), models [D][n], starting from 1, and the 8 stats - the host form, synchronous
ddcalIO :: GridHip -> GainSolve -> Int -> Int -> A.Vector Antenna -> A.Vector Antenna -> Maybe (A.Vector Antenna)
        -> Maybe (A.Vector F) -> A.Vector Visibility -> A.Matrix Visibility -> IO (A.Array A.DIM3 Visibility, [F])
ddcalIO h@(GridHip c) solve nant nslots ant1 ant2 slot wt vis models = do
  let A.Z A.:. n = A.arrayShape vis
      A.Z A.:. nd A.:. _ = A.arrayShape models
      (mode, ref, niter, tol) = solveCodes solve
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray (2 * nd * nslots * nant) :: IO (ForeignPtr CDouble)
  st <- withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withWt $ \ps -> withCplx vis $ \vs ->
          withCplx models $ \ms -> withForeignPtr out $ \po -> allocaArray 8 $ \pst -> do
            c_ddcal c (fi n) (fi nant) (fi nslots) (fi nd) a1 a2 sl vs ms ps mode ref 0 niter tol po pst >>= check h
            map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. nd A.:. nslots A.:. nant) (castForeignPtr out), st)

-- | ddSubtractIO h gains models directions ant1 ant2 slot vis: vis minus the corrupted models of the directions
-- (Nothing: all of them); vis Nothing: plus them, the corrupted model itself - the host form, synchronous
ddSubtractIO :: GridHip -> A.Array A.DIM3 Visibility -> A.Matrix Visibility -> Maybe [Int] -> A.Vector Antenna
             -> A.Vector Antenna -> Maybe (A.Vector Antenna) -> Maybe (A.Vector Visibility) -> IO (A.Vector Visibility)
ddSubtractIO h@(GridHip c) gains models directions ant1 ant2 slot vis = do
  let A.Z A.:. nd A.:. nslots A.:. nant = A.arrayShape gains
      A.Z A.:. _ A.:. n = A.arrayShape models
      dirs = maybe (2 ^ nd - 1) (sum . map (2 ^)) directions :: Int
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withVis k = maybe (k nullPtr) (\s -> withCplx s k) vis
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withCplx gains $ \g -> withCplx models $ \ms ->
    withVis $ \vs -> withForeignPtr out $ \po ->
      c_dd_subtract c (fi n) (fi nant) (fi nslots) (fi nd) a1 a2 sl g ms (fi dirs) vs po >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out))

-- ---------------------------------------------------------------------------------------------------------
-- Polarisation (include/gridhip.h, "polarisation"): a sample is four correlations, an [n][2][2] array; the gains are
-- [nslots][nant][2][2] Jones matrices.

-- | what a Jones solve solves for: a full 2x2 matrix per antenna, one gain per feed, or one phase per feed
data JonesMode = JonesFull | JonesDiagonal | JonesPhase

jonesModeCode :: JonesMode -> CInt
jonesModeCode JonesFull = 0
jonesModeCode JonesDiagonal = 1
jonesModeCode JonesPhase = 2

-- | jonescalIO h mode solve nant nslots ant1 ant2 slot wt vis model: the [nslots][nant][2][2] Jones matrices of
-- vis ~ G_p model G_q^H starting from the identity, and the 8 stats - the host form, synchronous.  gainPhaseOnly of
-- `solve` is not looked at: the mode says it.
jonescalIO :: GridHip -> JonesMode -> GainSolve -> Int -> Int -> A.Vector Antenna -> A.Vector Antenna
           -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Array A.DIM3 Visibility -> A.Array A.DIM3 Visibility
           -> IO (A.Array A.DIM4 Visibility, [F])
jonescalIO h@(GridHip c) jmode solve nant nslots ant1 ant2 slot wt vis model = do
  let A.Z A.:. n = A.arrayShape ant1
      (_, ref, niter, tol) = solveCodes solve
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray (8 * nslots * nant) :: IO (ForeignPtr CDouble)
  st <- withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withWt $ \ps -> withCplx vis $ \vs ->
          withCplx model $ \ms -> withForeignPtr out $ \po -> allocaArray 8 $ \pst -> do
            c_jonescal c (fi n) (fi nant) (fi nslots) a1 a2 sl vs ms ps (jonesModeCode jmode) ref 0 niter tol po pst
              >>= check h
            map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. nslots A.:. nant A.:. 2 A.:. 2) (castForeignPtr out), st)

-- | applyJonesIO h inverse gains ant1 ant2 slot wt vis: (the samples, the weights) after the Jones matrices - True: data
-- corrected, G_p^-1 vis G_q^-H with weights |det G_p| |det G_q| wt and weight 0 where there is no usable matrix; False:
-- a model corrupted, G_p vis G_q^H - the host form, synchronous
applyJonesIO :: GridHip -> Bool -> A.Array A.DIM4 Visibility -> A.Vector Antenna -> A.Vector Antenna
             -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Array A.DIM3 Visibility
             -> IO (A.Array A.DIM3 Visibility, A.Vector F)
applyJonesIO h@(GridHip c) inverse gains ant1 ant2 slot wt vis = do
  let A.Z A.:. n = A.arrayShape ant1
      A.Z A.:. nslots A.:. nant A.:. _ A.:. _ = A.arrayShape gains
      withSlot k = maybe (k nullPtr) (\s -> withI64 s k) slot
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
  out <- mallocForeignPtrArray (8 * n) :: IO (ForeignPtr CDouble)
  wout <- mallocForeignPtrArray n :: IO (ForeignPtr CDouble)
  withI64 ant1 $ \a1 -> withI64 ant2 $ \a2 -> withSlot $ \sl -> withWt $ \ps -> withCplx gains $ \g ->
    withCplx vis $ \vs -> withForeignPtr out $ \po -> withForeignPtr wout $ \pw ->
      c_apply_jones c (fi n) (fi nant) (fi nslots) a1 a2 sl g (if inverse then 1 else 0) vs ps po pw >>= check h
  return (A.fromForeignPtrs (A.Z A.:. n A.:. 2 A.:. 2) (castForeignPtr out), A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr wout))

-- | stokesIO h circular vis: the [4][n] block of the Stokes rows I, Q, U, V of the [n][2][2] samples (circular: the
-- basis is RR, RL, LR, LL, else XX, XY, YX, YY) - the host form, synchronous.  Each row is a scalar stream for an imager.
stokesIO :: GridHip -> Bool -> A.Array A.DIM3 Visibility -> IO (A.Matrix Visibility)
stokesIO h@(GridHip c) circular vis = do
  let A.Z A.:. n A.:. _ A.:. _ = A.arrayShape vis
  out <- mallocForeignPtrArray (8 * n) :: IO (ForeignPtr CDouble)
  withCplx vis $ \vs -> withForeignPtr out $ \po ->
    c_stokes c (fi n) (if circular then 1 else 0) 15 0 vs po >>= check h
  return (A.fromForeignPtrs (A.Z A.:. 4 A.:. n) (castForeignPtr out))

-- | imagerPeelIO im solve nant nslots ant1 ant2 slot wt model vis models: one peel step (gridhip_imager_peel_dev:
-- predict into row 0 of models, the direction-dependent solve, the subtraction of the directions 1 .. D - 1 and the
-- correction toward direction 0 as one chain on the device) -> (gains, the corrected visibilities, their weights, the
-- 8 stats)
imagerPeelIO :: ImagerH -> GainSolve -> Int -> Int -> A.Vector Antenna -> A.Vector Antenna
             -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Matrix F -> A.Vector Visibility
             -> A.Matrix Visibility -> IO (A.Array A.DIM3 Visibility, A.Vector Visibility, A.Vector F, [F])
imagerPeelIO (ImagerH h@(GridHip c) p n n') solve nant nslots ant1 ant2 slot wt model vis models = do
  let (mode, ref, niter, tol) = solveCodes solve
      A.Z A.:. nd A.:. _ = A.arrayShape models
      cells = nd * nslots * nant
      withSlot k = maybe (k nullPtr) (\s -> withI64 s $ \sp -> withDev h sp (8 * n) k) slot
  g <- mallocForeignPtrArray (2 * cells) :: IO (ForeignPtr CDouble)
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  wout <- mallocForeignPtrArray n :: IO (ForeignPtr CDouble)
  st <- withI64 ant1 $ \a1 -> withDev h a1 (8 * n) $ \d1 -> withI64 ant2 $ \a2 -> withDev h a2 (8 * n) $ \d2 ->
          withSlot $ \ds -> withDevWeights h n wt $ \dw -> withF model $ \mp -> withDev h mp (8 * n' * n') $ \dm ->
            withCplx vis $ \vs -> withDev h vs (16 * n) $ \dv -> withCplx models $ \ms ->
              withDev h ms (16 * nd * n) $ \dms -> withForeignPtr g $ \pg -> withDev h pg (16 * cells) $ \dg ->
                withForeignPtr wout $ \pw -> withDev h pw (8 * n) $ \dwo ->
                  withForeignPtr out $ \po -> allocaArray 8 $ \pst -> withDev h pst 64 $ \dst -> do
                    -- (the corrected visibilities in place, in the device copy of vis)
                    c_imager_peel_dev p dm dv (fi nant) (fi nslots) (fi nd) d1 d2 ds dw mode ref 0 niter tol dms dg dv dwo
                      dst >>= check h
                    c_memcpy_d2h c (castPtr pg) (castPtr dg) (fi (16 * cells)) >>= check h
                    c_memcpy_d2h c (castPtr po) (castPtr dv) (fi (16 * n)) >>= check h
                    c_memcpy_d2h c (castPtr pw) (castPtr dwo) (fi (8 * n)) >>= check h
                    c_memcpy_d2h c (castPtr pst) (castPtr dst) 64 >>= check h
                    c_synchronize c >>= check h
                    map realToFrac <$> peekArray 8 pst
  return (A.fromForeignPtrs (A.Z A.:. nd A.:. nslots A.:. nant) (castForeignPtr g),
          A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out), A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr wout), st)

-- ---------------------------------------------------------------------------------------------------------
-- Residual flagging (include/gridhip.h, "residual flagging"): robust per-group clipping of |vis - model|.

-- | how a flagging runs: nsigma of T = median + nsigma * 1.4826 MAD; amax (0: no limit); the fewest samples of a group
-- that is clipped; the most rounds (0 .. 16)
data FlagOptions = FlagOptions { flagNsigma :: F, flagAmax :: F, flagMinCount :: Int, flagNiter :: Int }

-- | flagResidualsIO h opts ngroups group wt vis model: (the weights with 0 where a sample is flagged, the class of every
-- sample, [n, median, MAD, T] per group, the 8 stats) - gridhip_flag_residuals, the host form, synchronous.  group
-- Nothing: one group (ngroups must be 1); wt Nothing: ones; model Nothing: zero.
flagResidualsIO :: GridHip -> FlagOptions -> Int -> Maybe (A.Vector Antenna) -> Maybe (A.Vector F) -> A.Vector Visibility
                -> Maybe (A.Vector Visibility) -> IO (A.Vector F, [Word8], [[F]], [F])
flagResidualsIO h@(GridHip c) (FlagOptions ns am mc ni) ngroups group wt vis model = do
  let A.Z A.:. n = A.arrayShape vis
      withGroup k = maybe (k nullPtr) (\s -> withI64 s k) group
      withWt k = maybe (k nullPtr) (\s -> withF s k) wt
      withModel k = maybe (k nullPtr) (\s -> withCplx s k) model
      rows xs = if null xs then [] else take 4 xs : rows (drop 4 xs)
  wout <- mallocForeignPtrArray (max 1 n) :: IO (ForeignPtr CDouble)
  (fl, gs, st) <- withGroup $ \pg -> withWt $ \ps -> withCplx vis $ \vs -> withModel $ \ms ->
    withForeignPtr wout $ \pw -> allocaArray (max 1 n) $ \pf -> allocaArray (4 * ngroups) $ \pgs -> allocaArray 8 $ \pst -> do
      c_flag_residuals c (fi n) (fi ngroups) pg vs ms ps (realToFrac ns) (realToFrac am) (fi mc) (fi ni) pw pf pgs pst
        >>= check h
      fl <- peekArray n pf
      gs <- map realToFrac <$> peekArray (4 * ngroups) pgs
      st <- map realToFrac <$> peekArray 8 pst
      return (fl, rows gs, st)
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr wout), fl, gs, st)

-- ---------------------------------------------------------------------------------------------------------
-- Direct-Fourier prediction (include/gridhip.h, "direct-Fourier prediction"): the exact visibilities of a component
-- list, and a model image as such a list.

-- | dftPredictIO h terms comps p x sub: sum_c S_c(x) E_c exp(-2 pi i (u l + v m + w (n - 1))) for the [C][10] component
-- rows {l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0} at the baselines p (wavelengths, not mirrored), or sub minus it, and the
-- 4 stats [used, skipped, non-finite visibilities, slices] - the host form, synchronous.  x Nothing: x = 0.
dftPredictIO :: GridHip -> Int -> A.Matrix F -> A.Vector BaseLines -> Maybe (A.Vector F) -> Maybe (A.Vector Visibility)
             -> IO (A.Vector Visibility, [F])
dftPredictIO h@(GridHip c) terms comps p x sub = do
  let A.Z A.:. n = A.arrayShape p
      A.Z A.:. ncomp A.:. _ = A.arrayShape comps
      withX k = maybe (k nullPtr) (\s -> withF s k) x
      withSub k = maybe (k nullPtr) (\s -> withCplx s k) sub
  out <- mallocForeignPtrArray (2 * n) :: IO (ForeignPtr CDouble)
  st <- withF comps $ \pc -> withUVW p $ \pu pv pw -> withX $ \px -> withSub $ \ps -> withForeignPtr out $ \po ->
          allocaArray 4 $ \pst -> do
            c_dft_predict c (fi ncomp) pc nullPtr (fi terms) (fi n) pu pv pw 1 px ps po pst >>= check h
            map realToFrac <$> peekArray 4 pst
  return (A.fromForeignPtrs (A.Z A.:. n) (castForeignPtr out), st)

-- | componentsFromImageIO h theta lam terms maxc model: the non-zero cells of the [terms][N][N] model as point components
-- in row-major order -> (the [maxc][10] rows, of which the first min found maxc are written, the number found)
componentsFromImageIO :: GridHip -> F -> Int -> Int -> Int -> A.Array A.DIM3 F -> IO (A.Matrix F, Int)
componentsFromImageIO h@(GridHip c) theta lam terms maxc model = do
  out <- mallocForeignPtrArray (10 * maxc) :: IO (ForeignPtr CDouble)
  found <- withF model $ \pm -> withForeignPtr out $ \po -> alloca $ \pn -> do
             mapM_ (\i -> pokeElemOff po i 0) [0 .. 10 * maxc - 1]
             c_components_from_image c (realToFrac theta) (fi lam) (fi terms) pm (fi maxc) po pn >>= check h
             fromIntegral <$> peek pn
  return (A.fromForeignPtrs (A.Z A.:. maxc A.:. 10) (castForeignPtr out), found)

-- ---------------------------------------------------------------------------------------------------------
-- Source finding (include/gridhip.h, "source finding"): a map as a list of Gaussian components.

-- | findSourcesIO h theta lam opts sigma border beam correct maxc image: the islands of the N x N map under the levels of
-- opts (amAbsolute and amGrow are not used), each measured by its moments -> (the [maxc][10] component rows that
-- dftPredictIO takes, of which the first min found maxc are written, the [maxc][16] measurements, the number found, the 8
-- stats [T_hi, T_lo, P, found, written, points, summed flux, reason]).  beam: the 8 values of fitBeamIO, or Nothing -
-- gridhip_find_sources, the host form, synchronous
findSourcesIO :: GridHip -> F -> Int -> AutomaskOptions -> F -> Int -> Maybe [F] -> Bool -> Int -> A.Matrix F
              -> IO (A.Matrix F, A.Matrix F, Int, [F])
findSourcesIO h@(GridHip c) theta lam (AutomaskOptions _ (th, tl) (nh, nl) pf mc _) sigma border beam correct maxc image = do
  out <- mallocForeignPtrArray (10 * maxc) :: IO (ForeignPtr CDouble)
  inf <- mallocForeignPtrArray (16 * maxc) :: IO (ForeignPtr CDouble)
  let withBeam k = maybe (k nullPtr) (\b -> withArray (map realToFrac b :: [CDouble]) k) beam
  (found, st) <- withF image $ \pi' -> withForeignPtr out $ \po -> withForeignPtr inf $ \pq ->
    with (realToFrac sigma :: CDouble) $ \pn -> withBeam $ \pb -> alloca $ \pc -> allocaArray 8 $ \ps -> do
      mapM_ (\i -> pokeElemOff po i 0) [0 .. 10 * maxc - 1]
      mapM_ (\i -> pokeElemOff pq i 0) [0 .. 16 * maxc - 1]
      c_find_sources c (realToFrac theta) (fi lam) pi' (fi border) (realToFrac th) (realToFrac tl) (realToFrac nh)
        (realToFrac nl) pn (realToFrac pf) (fi mc) pb (if correct then 1 else 0) (fi maxc) po pq pc ps >>= check h
      n <- fromIntegral <$> peek pc
      s <- map realToFrac <$> peekArray 8 ps
      return (n, s)
  return ( A.fromForeignPtrs (A.Z A.:. maxc A.:. 10) (castForeignPtr out)
         , A.fromForeignPtrs (A.Z A.:. maxc A.:. 16) (castForeignPtr inf), found, st )

-- ---------------------------------------------------------------------------------------------------------
-- A whole node from one Haskell process: ndev devices, visibilities cut into contiguous shards, partial grids
-- summed with one RCCL all-reduce over xGMI (include/gridhip.h, gridhip_comm_*).

withNode :: Int -> (Node -> IO a) -> IO a
withNode ndev = bracket open (\(Node c) -> () <$ c_comm_destroy c)
  where open = alloca $ \pp -> do
                 rc <- c_comm_create (fi ndev) nullPtr pp
                 when (rc /= 0) $ c_comm_last_error nullPtr >>= peekCString >>= error
                 Node <$> peek pp

-- | convgrid2 over all devices of the node (same arguments and result as convgrid2IO)
convgrid2NodeIO :: Node -> A.Array A.DIM5 Visibility -> A.Matrix Visibility -> A.Vector BaseLines
                -> A.Vector Int -> A.Vector Visibility -> IO (A.Matrix Visibility)
convgrid2NodeIO (Node c) gcf a p wbin v = do
  (out, hgt, wid) <- copyGrid a
  let A.Z A.:. w A.:. q A.:. _ A.:. gh A.:. gw = A.arrayShape gcf
      A.Z A.:. n = A.arrayShape v
  rc <- withForeignPtr out $ \o -> withCplx gcf $ \k -> withUVW p $ \pu pv _ -> withI wbin $ \wb -> withCplx v $ \vs ->
          c_comm_convgrid2 c (fi hgt) (fi wid) o (fi n) (fi w) (fi q) (fi gh) (fi gw) k pu pv 1 wb vs
  when (rc /= 0) $ c_comm_last_error c >>= peekCString >>= \m -> error ("gridhip node: " ++ m)
  return (adoptGrid out hgt wid)
