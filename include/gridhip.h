/*
 * gridhip.h — C ABI of libgridhip.so: MI355X (gfx950 / CDNA4) native convolutional
 * w-projection gridder / degridder.
 *
 * This is the drop-in boundary for the gridding hot path of
 * sakehl/SKA-SDP-Accelerate-gridding.  Each entry point replaces the *body* of one
 * Accelerate function of /root/reference/src/Gridding.hs (cited per function); the Haskell
 * signatures stay, the `run` over the array program becomes a `foreign import ccall` into
 * this library (binding shown in INTEGRATION.md).
 *
 * Conventions (all follow the reference's own FFI style, hdf5/hdf5.cc:59-186 and
 * src/Hdf5.hs:30-67: extern "C", plain pointers + integers, caller allocates outputs):
 *   F = double, Int = int64_t, Antenna = int64_t            (src/Types.hs:7-16)
 *   Complex Double arrays = interleaved (re,im) doubles     (src/Hdf5.hs:113-137, hdf5/hdf5.cc:14-17)
 *   Vector (F,F,F) = separate u / v / w pointers; `uv_stride` is the element stride between
 *       consecutive visibilities (1 for struct-of-arrays as Accelerate stores tuples, 3 when u
 *       and v point into the (n,3) row-major /vis/uvw matrix, src/ImageDataset.hs:94-97)
 *   grids are row-major [y][x] (y <-> v axis), H rows x Wd columns (src/Gridding.hs:106-109)
 *   gcf   = [W][Q][Q][gh][gw] complex, index order (wbin, yf, xf, i, j) (src/Gridding.hs:243)
 *   grids are ACCUMULATED INTO (permute (+) a ..., src/Gridding.hs:99,197,244), never overwritten
 *   the library never retains or frees a caller pointer past the call
 *
 * Every function returns GRIDHIP_OK (0) or a negative GRIDHIP_E* code; the message for the
 * last failure on a context is available from gridhip_last_error().  (The reference's FFI
 * reports nothing; this is the one deliberate departure)
 *
 * Two flavours per operation:
 *   gridhip_<op>      host pointers, synchronous — the drop-in form.  It stages its arrays through device blocks
 *                     from a pool the context keeps: a repeated call of a shape allocates nothing, and the blocks
 *                     stay allocated until gridhip_destroy;
 *   gridhip_<op>_dev  device pointers, asynchronous on the context's stream — what the
 *                     benchmark and multi-GPU drivers use so that H2D is outside the timing.
 *                     `grid` and `vis_out` must be ordinary device allocations (hipMalloc: coarse-grained
 *                     memory): the tile kernels flush with hardware fp64 atomics (global_atomic_add_f64),
 *                     which fine-grained / host-coherent mappings do not support.
 * A context is bound to one device and one stream and is not thread-safe; contexts are independent of each other (one
 * per host thread: tests/test_gpu_limits.py runs two on one GPU concurrently).
 */
#ifndef GRIDHIP_H
#define GRIDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRIDHIP_VERSION 320 /* 0.3.2 */

#define GRIDHIP_OK 0
#define GRIDHIP_EINVAL (-1)       /* bad argument (null pointer, negative size, ...) */
#define GRIDHIP_ENOMEM (-2)       /* device or host allocation failed */
#define GRIDHIP_EHIP (-3)         /* HIP runtime / library error, see gridhip_last_error */
#define GRIDHIP_ENODEV (-4)       /* no usable gfx950 device */
#define GRIDHIP_EUNSUPPORTED (-5) /* shape outside what the kernels support */

typedef struct gridhip_ctx gridhip_ctx;

/* ---- context --------------------------------------------------------------------------- */
int gridhip_version(void);
const char *gridhip_strerror(int code);
int gridhip_device_count(int *count);
/* Create a context on HIP device `device` with its own non-blocking stream. */
int gridhip_create(int device, gridhip_ctx **ctx);
int gridhip_destroy(gridhip_ctx *ctx);
const char *gridhip_last_error(const gridhip_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL means HIP's default
 * (null) stream, NOT "no stream": device-pointer calls must be ordered with the caller's own
 * kernels and copies, and those run on the null stream unless the caller created another.
 * gridhip_reset_stream() goes back to the context's private non-blocking stream (which does not
 * synchronise with the null stream: only use it when the inputs are known to be complete). */
/* A context has ONE set of scratch buffers (records, tables, sorted lists, padded kernels): when the stream changes,
 * the new stream is made to wait (event) for what was enqueued on the old one, so a caller that alternates streams
 * between calls cannot have one call overwrite scratch another is still reading.  (Not while either stream is being
 * captured into a graph: a capture must not depend on work outside it - use one stream per context there.) */
int gridhip_set_stream(gridhip_ctx *ctx, void *hip_stream);
int gridhip_reset_stream(gridhip_ctx *ctx);
void *gridhip_get_stream(gridhip_ctx *ctx);
int gridhip_synchronize(gridhip_ctx *ctx);
/* Tuning knobs (all have defaults chosen per shape):
 *   "tile"      side of a square grid tile in cells (8..128; 0 = auto: the largest rectangle whose planes fit the
 *               LDS layout, 65 x 89 cells for a 15 x 15 kernel); "tile_x" / "tile_y": a rectangular tile
 *   "block"     threads per work-group of the tile kernels (multiple of 64, <=1024; 0 = auto)
 *   "chunk"     max visibilities per work item (0 = auto; the sorted kernel takes at most 16384)
 *   "wgroups"   number of w-plane groups work items are split into for XCD/L2 locality (1..16; 0 = auto)
 *   "variant"   0 = LDS-tile accumulate (default), 1 = direct global-atomic scatter (baseline)
 *   "sort"      order each work item's records by kernel slice so that runs of visibilities
 *               reuse their taps from registers: 0 = auto, 1 = on (when the shape allows), 2 = off
 *   "prepass"   scatter of the binning pre-pass: 0 = auto (two levels from 2^22 visibilities), 1 = one level,
 *               2 = two levels (the counting sweep leaves 8-byte pre-records, which are LDS-sorted into runs per
 *               coarse bin and then per bin), 3 = one level with global atomics only (no LDS; a measured
 *               baseline), 4 = two levels recomputing from the stream instead of reading pre-records,
 *               5, 6 = two levels with 16-byte / 12-byte instead of 8-byte intermediate records
 *   "coarse_shift", "scatter_chunk", "count_unroll"  details of that scatter kept for comparison runs: bins per
 *               coarse bin = 2^coarse_shift (0 = balanced); scatter_chunk = 4096: half-size chunks, two work-groups
 *               per CU; count_unroll = 4: four visibilities per thread and trip in the counting sweep, 1: one, and
 *               no 16-byte grid-stride form either (0 = auto)
 *   "bin_reuse" 0 = auto: a convgrid2 / degrid2 call whose geometry, n, stride, u / v / wbin pointers and pre-pass options
 *               equal the previous call's, with no other pre-pass on the context in between, first verifies in one
 *               read-only sweep that every visibility still falls into the same bin, cell and kernel slice, and if so
 *               keeps the previous call's binned records instead of running the two scatter levels (the values may
 *               change freely; results are those of a full pre-pass either way; after a failed attempt the next 4
 *               calls do not try); 1 = never.  A call made while the stream is being captured into a graph neither
 *               verifies nor leaves anything to reuse, and a replay of such a graph marks the device so that the
 *               next call after it runs its pre-pass in full
 *   "list_reuse" 0 = auto: such a call over the two-level pre-pass also keeps the tap-reusing tile kernel's per-work-item
 *               lists of records sorted by kernel slice (in the block that held the pre-records, 8 B per record), and the
 *               next one whose records stand - same work-item shape, no other pre-pass in between, the verify sweep's
 *               verdict read on the device - walks them instead of sorting again (convgrid2 and degrid2 share them, as
 *               they share the records); 1 = never: every call sorts into the per-work-group scratch.  Calls cut into
 *               parts, the one-level pre-pass, the aw forms, plans, imagers and captured calls always do; "bin_reuse" = 1
 *               implies it
 *   "aw_cache"  aw gridders: 1 (default) = build each distinct (a1, a2, wbin, yf, xf) kernel once per call and let
 *               the visibilities that share it reuse it; 0 = one kernel per visibility (as the reference evaluates)
 *   "aw_batch"  aw gridders, degridders and plans: visibilities per batch of the kernel table.  0 (default) = 2^20 with
 *               "aw_cache", 2^22 without; k > 0 = min(k, that).  For tests of the batch loop and for bounding the scratch
 *               memory (one S x S kernel per visibility of a batch).  The one option that can be set negative: every aw
 *               entry point then returns GRIDHIP_EINVAL before it touches anything.  A plan keeps the batches it was made with
 *   "fault_inject"  TEST HOOK: hides the last k slots of the record array from the pre-pass's scatter so that its
 *               bounds checks have something to reject (counted in "errors"; results are then incomplete)
 *   "reserve_cus"  compute units the persistent tile kernel leaves free (0 = none): it launches one work-group per
 *               remaining CU, so that a collective queued on another stream (RCCL's kernel, a copy) finds CUs to start
 *               on while the tile kernel runs instead of waiting ~10 ms for it to end; costs the tile kernel
 *               k / num_cu of its throughput (profiles/r03_reserve_cus.txt)
 *   "yield_cus"  the cheaper way to the same end (0 = off; ignored while "reserve_cus" is set): k CUs' worth of the tile
 *               kernel's work-groups are not persistent - each takes eight work items and leaves, and up to 2 048
 *               further ones are launched to follow them - so a kernel queued on another stream gets a CU within a few
 *               hundred microseconds while nothing idles when none is queued (+0.5 % on the tile kernel instead of
 *               +10 %).  k is rounded up to a multiple of 32 (one CU per shader engine of every XCD): with fewer the
 *               dispatcher's rotation over the shader engines stops at one without a free CU and the CUs given up stay
 *               idle (profiles/r03_yield_cus.txt)
 *   "bigtile"   the tap-reusing kernel's tile uses all of the LDS (65 x 110 cells at 15 x 15 instead of 65 x 89): a
 *               quarter more visibilities per kernel slice and work item, for an address add per tap step; pays
 *               where items are sparse (fewer than two visibilities per slice and item), not where the LDS atomic
 *               unit binds.  0 = auto (sparse streams of at least 2^22 visibilities), 1 = on, 2 = off
 *   "subfoot"   1 = supports 17..32 take the sub-footprint path (one record per spatial part of the kernel, as
 *               supports above 32 and non-square kernels always do) instead of the tap-reusing kernel's own parts of
 *               the tap list (one record per visibility): kept for comparison runs
 *   "wtable"    which table of walker weights the tap-reusing kernel uses: 0 = auto, 1 = flat, 2 = steep (tile_sorted.hip)
 *   "rec_bits"  TEST HOOK: pretend the 64-bit record word has this many bits (16..63), so that small calls take the
 *               path that grids a call in several parts (taken for real above 2^50 slices x visibilities);
 *               100 + t: widen the record's kernel-slice field until its fields take t <= 64 bits
 *   "dft_slices"  gridhip_dft_predict: the slices S the component list is cut into; 0 = auto (a function of n and C
 *               alone), 1..64 = that many (values above 64 count as 64)
 *   "sources_deblend"  gridhip_find_sources and its _dev and imager forms: 0 (default) = an island is one row; r in 1..32 =
 *               an island is split into one row per peak, with window radius r cells ("source finding", DEBLENDING).  Read
 *               when a call is enqueued.  A value above 32 is kept as given: the three entry points then return
 *               GRIDHIP_EINVAL before they touch anything
 *   "mosaic_cull"  gridhip_mosaic: 0 = every tile walks the facets its cull keeps, 1 = every tile walks all valid facets
 *               (the same bits: kept for comparison runs)
 *   "rm_stage"  gridhip_rmclean: 0 = every wave reads and writes its line of sight directly, 1 = a work-group moves its
 *               lines of sight through LDS, consecutive threads along m (the same bits: kept for comparison runs)
 *   "noisemap_hist"  gridhip_noise_map: how the node kernel builds the 256-counter histogram of a pass.  0 (default) =
 *               every lane adds to one copy; else bits: 1 = skip the digits that the window's smallest and largest key
 *               share, 2 = one copy of the counters per wave, 4 = lanes of a wave with the same digit add once (up to
 *               four digits per step).  The same bits each way, and each slower than 0 where measured: kept for
 *               comparison runs
 *   "wstack_middle"  gridhip_imager_cycle_dev of an imager of kind 4 (w-stacking): 0 (default) = the pass over the
 *               visibilities between the prediction and the gridding runs once, in the layer order of the mirrored
 *               stack; 1 = it runs in stream order between the stacks' two permuting passes (three passes over the
 *               visibilities instead of one).  The same vis_res bit for bit and images equal to the atomics' tolerance;
 *               0 is the faster where measured, 1 is kept for comparison runs.  Read per call.
 *   "scratch_fill"  TEST HOOK: 0 (default) = off; 1..255 = every block of device memory the library takes for itself - a
 *               pooled block each time it is handed out (scratch and the host-pointer forms' staging alike), a gridder
 *               workspace when it grows, the blocks a plan, stack or imager owns - is first filled with this byte, in
 *               stream order, so that a kernel that reads scratch it never wrote, or a host form that returns an output
 *               it filled only in part, shows.  Values above 255 are refused.  Set it before the context's first call.
 *               Each fill is a memset node: not for calls captured into a graph.  Memory from gridhip_malloc is the
 *               caller's and is left alone
 *   ("dbg", the ablation / profiling switch of tuning runs, exists only in the tuning build of the library,
 *   `make -C csrc tuning` -> lib/libgridhip_tuning.so; the shipped library rejects the key)
 * Read-only (gridhip_get_option): "prepass_verified" = calls so far that ran the verify sweep of "bin_reuse",
 * "prepass_reused" = those of them that kept their records (counted on the device: reading it synchronises the stream);
 * "lists_reused" = tile launches so far that were told the previous call's sorted lists are in place ("list_reuse"; the
 * kernel still sorts afresh if the verify sweep then finds the records changed);
 * "scratch_filled" = blocks filled so far on this context by the test hook "scratch_fill";
 * "idg_chunk", "idg_split" = the visibilities the image-domain gridder ("w-stacking", IMAGE-DOMAIN LAYERS) stages in LDS at
 * a time, and the size above which a tile's visibilities are cut into several work items;
 * "last_wgroups", "last_tile_x", "last_tile_y", "last_bigtile" = the geometry the last convgrid / convgrid2 / degrid2
 * call chose (w-groups, the LDS tile's interior, whether the tile uses all of the LDS);
 * "aw_tables_built" = kernel tables (one per batch of visibilities) the last aw gridding / degridding / imaging call or
 * aw plan or aw imager creation built (0 after an aw plan pass or an imager's cycle);
 * "last_path" = which gridder the last convgrid / convgrid2 / degrid2 / plan / aw gridding (convgrid4, aw_imaging and the
 * other calls that run the aw batch loop) / awdegrid / aw plan pass call used:
 * 1 = the tap-reusing tile kernel (square supports 5..32 with enough visibilities per work item), 2 = the same through
 * sub-footprints (other shapes: one record per spatial part of the kernel), 3 = the general tile kernel (small
 * problems, and the sizes listed under "Limits" below: 2 - 3 x slower per visibility at scale), 4 = direct
 * global-atomic scatter; "errors" = internal consistency failures counted by the last tile-kernel
 * launch (expected 0); "clock_khz" = shader clock held during the last tap-reusing tile kernel (in-kernel
 * s_memtime / s_memrealtime stamps), "aw_clock_khz" = the same for the last launch of the aw gridders' kernel builder; "prof0".."prof31" = cycle counters of a dbg=16 launch of the tuning build (tools/phase_profile.py).
 */
int gridhip_set_option(gridhip_ctx *ctx, const char *key, int64_t value);
int gridhip_get_option(gridhip_ctx *ctx, const char *key, int64_t *value);
/* Visibilities skipped by the last gridding call because `wbin` was outside [0,W) (the
 * reference would read the kernel out of range).  Synchronises the stream. */
int gridhip_last_dropped(gridhip_ctx *ctx, int64_t *dropped);

/* ---- Limits ------------------------------------------------------------------------------------
 * Per call: n < 2^31 - 256 visibilities (GRIDHIP_EUNSUPPORTED above; cut the stream), H, Wd <= 2^30, W * Q * Q <= 2^30,
 * gh, gw <= 1024.  A kernel that is not a square of side 5..32 is gridded as P = py * px sub-footprints, one binned
 * record per part, which needs n * P < 2^31 - 256 and W * Q * Q * P < 2^30: a call beyond either takes the general
 * tile kernel instead (read-only option "last_path" = 3 says so; nothing is lost but speed) - cut the stream into
 * calls of fewer visibilities to stay on the fast path.  Slices x visibilities above 2^50 are gridded in several
 * parts internally.  degrid2 has no direct form: a support too large for an LDS tile is GRIDHIP_EUNSUPPORTED. */

/* ---- gridders: host pointers (drop-in) -------------------------------------------------- */

/* grid  — src/Gridding.hs:95-112.   G[N/2+floor(.5+N*v), N/2+floor(.5+N*u)] += vis
 * (N = H as in the reference, :101-103; cells outside the grid are dropped). */
int gridhip_grid(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                 const double *u, const double *v, int64_t uv_stride, const double *vis);

/* convgrid — src/Gridding.hs:153-197.  gcf is [Q][Q][gh][gw]. */
int gridhip_convgrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                     int64_t Q, int64_t gh, int64_t gw, const double *gcf, const double *u,
                     const double *v, int64_t uv_stride, const double *vis);

/* convgrid2 — src/Gridding.hs:199-244 (the w-projection kernel).  gcf is [W][Q][Q][gh][gw]. */
int gridhip_convgrid2(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                      int64_t W, int64_t Q, int64_t gh, int64_t gw, const double *gcf,
                      const double *u, const double *v, int64_t uv_stride,
                      const int64_t *wbin, const double *vis);

/* degrid2 — the gather with convgrid2's coordinates (north_star "degrid"; absent from the
 * reference, defined in SURVEY.md §8a): vis_out[k] = sum_ij gcf[wbin,yf,xf,i,j]*G[y0+i,x0+j]. */
int gridhip_degrid2(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid, int64_t n,
                    int64_t W, int64_t Q, int64_t gh, int64_t gw, const double *gcf,
                    const double *u, const double *v, int64_t uv_stride,
                    const int64_t *wbin, double *vis_out);

/* ---- gridders: device pointers, asynchronous on the context's stream --------------------- */
int gridhip_grid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                     const double *u, const double *v, int64_t uv_stride, const double *vis);
int gridhip_convgrid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                         int64_t Q, int64_t gh, int64_t gw, const double *gcf,
                         const double *u, const double *v, int64_t uv_stride,
                         const double *vis);
int gridhip_convgrid2_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n,
                          int64_t W, int64_t Q, int64_t gh, int64_t gw, const double *gcf,
                          const double *u, const double *v, int64_t uv_stride,
                          const int64_t *wbin, const double *vis);
int gridhip_degrid2_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid,
                        int64_t n, int64_t W, int64_t Q, int64_t gh, int64_t gw,
                        const double *gcf, const double *u, const double *v,
                        int64_t uv_stride, const int64_t *wbin, double *vis_out);

/* ---- plans: bin the baselines once, grid / degrid many times (device pointers) ----------------
 * The binning pre-pass depends on (u, v, wbin) and the kernel-table SHAPE only.  do_imaging grids
 * the same baselines twice (image and PSF, src/Gridding.hs:538,541) and major cycles alternate
 * degrid / grid over them; a plan keeps the tile-ordered records resident so each further pass is
 * the tile kernel alone.  The coordinate arrays may be released after gridhip_plan_create_dev
 * returns and the stream has run; vis / grid / gcf are per call.  A plan belongs to its context
 * (same device, same stream, not thread-safe) and must be destroyed before it. */
typedef struct gridhip_plan gridhip_plan;
int gridhip_plan_create_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, int64_t n, int64_t W, int64_t Q,
                            int64_t gh, int64_t gw, const double *u, const double *v,
                            int64_t uv_stride, const int64_t *wbin, gridhip_plan **plan);
int gridhip_plan_grid_dev(gridhip_plan *plan, const double *gcf, const double *vis, double *grid);
int gridhip_plan_degrid_dev(gridhip_plan *plan, const double *gcf, const double *grid,
                            double *vis_out);
int gridhip_plan_destroy(gridhip_plan *plan);

/* ---- callers either side of the gridder (host pointers) -------------------------
 * All follow src/Gridding.hs; uvw are in wavelengths where the reference takes them so. */

/* N = round (theta * lam) as the imaging functions compute it (:87,:118,:416; Prelude round). */
int64_t gridhip_image_size(double theta, int64_t lam);
/* w-bin rule of w_cache_imaging, :426-432: wbin = (wstep*round(w/wstep) - min) div wstep. */
int gridhip_wbins(gridhip_ctx *ctx, int64_t n, const double *w, int64_t wstep, int64_t *wbin,
                  int64_t *wmin, int64_t *nplanes);
/* findClosest, :895-907, for each w (out of range reads clamped as ImageDataset.hs:150-168). */
int gridhip_find_closest(gridhip_ctx *ctx, int64_t nws, const double *ws, int64_t n,
                         const double *w, int64_t *out);
/* mirror_uvw, :551-562, in place (w and vis may be NULL). */
int gridhip_mirror_uvw(gridhip_ctx *ctx, int64_t n, double *u, double *v, double *w, double *vis);
/* doweight, :564-583: vis /= number of visibilities in its grid cell; u, v in wavelengths. */
int gridhip_doweight(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u,
                     const double *v, double *vis);
/* make_grid_hermitian, :585-605, in place. */
int gridhip_make_grid_hermitian(gridhip_ctx *ctx, int64_t N, double *grid);
/* fft / ifft, :815-829: shift2D . fft2D . ishift2D on an N x N complex array (hipFFT);
 * inverse != 0 is scaled by 1/N^2 as accelerate-fft's Inverse mode. */
int gridhip_fft2_centered(gridhip_ctx *ctx, int64_t N, const double *in, double *out, int inverse);
/* w_kernel, :610-728: out is [qpx][qpx][npixKern][npixKern].
 * The w-kernel shape rule, GRIDHIP_EINVAL before anything is touched (out is left as it was): npixFF, npixKern, qpx >= 1,
 * npixKern <= npixFF, and with na = npixFF * qpx
 *     na / 2 - qpx * (npixKern / 2) >= qpx - 1        (integer divisions)
 * extract_oversampled (:709-728) reads the transformed na x na far field from row and column
 * na / 2 - qpx * (npixKern / 2) - (qpx - 1) on; the reference indexes outside its array where that is negative, e.g.
 * (npixFF, npixKern, qpx) = (8, 8, 2) or (16, 16, 2); (9, 9, 2) and every qpx = 1 shape are legal.  The rule holds for
 * every entry point that takes (npixFF, npixKern, qpx): this one and the w_cache kind (kind 2) of w_cache_imaging,
 * do_imaging, predict and the imagers, host and _dev forms alike. */
int gridhip_w_kernel(gridhip_ctx *ctx, double theta, double w, int64_t npixFF, int64_t npixKern,
                     int64_t qpx, double *out);
/* ImagingFunctions (:76-81): grid is N x N with N = gridhip_image_size(theta, lam), overwritten. */
int gridhip_simple_imaging(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u,
                           const double *v, int64_t uv_stride, const double *vis, double *grid);
int gridhip_conv_imaging(gridhip_ctx *ctx, int64_t Q, int64_t gh, int64_t gw, const double *kv,
                         double theta, int64_t lam, int64_t n, const double *u, const double *v,
                         int64_t uv_stride, const double *vis, double *grid);
/* w_cache_imaging, :399-449: builds one conjugated w_kernel per plane, then convgrid2.  (qpx, npixFF, npixKern):
 * the w-kernel shape rule stated at gridhip_w_kernel. */
int gridhip_w_cache_imaging(gridhip_ctx *ctx, int64_t wstep, int64_t qpx, int64_t npixFF,
                            int64_t npixKern, double theta, int64_t lam, int64_t n, const double *u,
                            const double *v, const double *w, int64_t uv_stride, const double *vis,
                            double *grid);
/* convgrid3 / convgrid4, :246-396 (both produce this grid): per visibility
 * awkern = conj(aw_kernel_fn2 yf xf wkerns[wbin] akerns[a1] akerns[a2]) (:761-775, convolve2d :795-811 with
 * its transposing pad), G[y0+i,x0+j] += vis*awkern[i,j].  wkerns [W][Q][Q][S][S], akerns [A][S][S];
 * the index triple (wbin, a1, a2) is passed as three arrays (Accelerate's struct-of-arrays).
 * The kernel of every distinct (a1, a2, wbin, yf, xf) is built once per call (option "aw_cache"). */
int gridhip_awgrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n, int64_t W,
                   int64_t Q, int64_t S, int64_t A, const double *wkerns, const double *akerns,
                   const double *u, const double *v, int64_t uv_stride, const int64_t *wbin,
                   const int64_t *a1, const int64_t *a2, const double *vis);
int gridhip_awgrid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n, int64_t W,
                       int64_t Q, int64_t S, int64_t A, const double *wkerns, const double *akerns,
                       const double *u, const double *v, int64_t uv_stride, const int64_t *wbin,
                       const int64_t *a1, const int64_t *a2, const double *vis);
/* What the last gridhip_awgrid / gridhip_awgrid_dev / gridhip_awdegrid* / gridhip_aw_plan_create_dev call on this
 * context did (synchronises): visibilities that received a kernel, and distinct (a1, a2, wbin, yf, xf) kernels built
 * for them (equal with "aw_cache" = 0). */
int gridhip_aw_last_stats(gridhip_ctx *ctx, int64_t *vis_keyed, int64_t *kernels_built);
/* awdegrid — the gather that matches convgrid4's scatter (absent from the reference, like degrid2; parity is
 * unpinned there): the same coordinates (frac_coords, the half-support shift) and the same kernel the gridder scatters,
 *     awkern_k   = conj(aw_kernel_fn2(yf_k, xf_k, wkerns[wbin_k], akerns[a1_k], akerns[a2_k]))   (:761-775)
 *     vis_out[k] = sum_ij awkern_k[i,j] * G[y0_k+i, x0_k+j]      (taps outside the grid contribute 0)
 * i.e. the gridding kernel as given, not conjugated (degrid2's convention).  Adjoint identity:
 * vdot(g, awgrid(wk, ak, vis)) == vdot(awdegrid(conj wk, conj ak, g), vis).  vis_out is overwritten, not accumulated;
 * a visibility whose wbin, a1 or a2 is out of range predicts exactly 0 and is counted (gridhip_last_dropped), as the
 * aw gridder counts it.  Limits and errors are gridhip_awgrid's; a support the LDS tile cannot hold for a gather is
 * GRIDHIP_EUNSUPPORTED, as for degrid2.  "last_path" = 1 (tap-reusing tile kernel, square supports 5..16) or 3
 * (general tile kernel).  The host form is synchronous, the _dev form takes device pointers and is asynchronous.
 * The host forms of awgrid and awdegrid keep their staging blocks in the context's pool between calls, as every
 * other host form does (gridhip_destroy frees them). */
int gridhip_awdegrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid, int64_t n, int64_t W,
                     int64_t Q, int64_t S, int64_t A, const double *wkerns, const double *akerns,
                     const double *u, const double *v, int64_t uv_stride, const int64_t *wbin,
                     const int64_t *a1, const int64_t *a2, double *vis_out);
int gridhip_awdegrid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid, int64_t n, int64_t W,
                         int64_t Q, int64_t S, int64_t A, const double *wkerns, const double *akerns,
                         const double *u, const double *v, int64_t uv_stride, const int64_t *wbin,
                         const int64_t *a1, const int64_t *a2, double *vis_out);
/* ---- aw plans: key, build and bin the baselines once, grid / degrid many times (device pointers) --------------
 * An aw call spends most of its time building its table of distinct kernels from wkerns / akerns (2.7 - 2.8 of 3.1 ms
 * at 10^6 visibilities, 4096^2, 15 x 15), and a major cycle re-grids and re-predicts the same baselines with the same
 * kernels.  Unlike gridhip_plan, an aw plan therefore CAPTURES THE KERNEL VALUES: it keeps, per batch of 2^20
 * visibilities, the binned records, the bin / work tables and the batch's table of distinct kernels (compacted to
 * the batch's distinct count).  Every input of create may be freed or overwritten once create has returned; create
 * synchronises the stream (it reads each batch's distinct count to size that batch's table).  Passes are asynchronous,
 * build nothing ("aw_tables_built" reads 0 after one) and set "last_path" as awdegrid does.  plan_grid_dev ACCUMULATES
 * into grid (convgrid4); plan_degrid_dev overwrites vis_out (awdegrid).  gridhip_aw_last_stats and
 * gridhip_last_dropped report the plan's creation.  Limits and errors are gridhip_awgrid's (a support the LDS tile
 * cannot hold for a gather: GRIDHIP_EUNSUPPORTED).  A plan belongs to its context (same device, same stream, not
 * thread-safe) and must be destroyed before it. */
typedef struct gridhip_aw_plan gridhip_aw_plan;
int gridhip_aw_plan_create_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, int64_t n, int64_t W, int64_t Q,
                               int64_t S, int64_t A, const double *wkerns, const double *akerns,
                               const double *u, const double *v, int64_t uv_stride, const int64_t *wbin,
                               const int64_t *a1, const int64_t *a2, gridhip_aw_plan **plan);
int gridhip_aw_plan_grid_dev(gridhip_aw_plan *plan, const double *vis, double *grid);
int gridhip_aw_plan_degrid_dev(gridhip_aw_plan *plan, const double *grid, double *vis_out);
int gridhip_aw_plan_destroy(gridhip_aw_plan *plan);
/* aw_imaging / aw_imagingOld, :452-506: wvals are the W plane w-values searched by findClosest. */
int gridhip_aw_imaging(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                       int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                       int64_t n, const double *u, const double *v, const double *w,
                       int64_t uv_stride, const int64_t *a1, const int64_t *a2, const double *vis,
                       double *grid);
/* aw_imaging with every array argument resident on the device (wkerns, wvals, akerns, u, v, w, a1, a2, vis in; the
 * N x N grid out, overwritten): replaces the `run` of :452-478 as gridhip_aw_imaging does, but asynchronous on the
 * context's stream and reading nothing back.  One front-end kernel reads the strided u, v, w once (p = uvw / lam,
 * findClosest of w in wavelengths), then the aw gridder.  a1 / a2 are taken as given. */
int gridhip_aw_imaging_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                           const double *wkerns, const double *wvals, const double *akerns, int64_t n,
                           const double *u, const double *v, const double *w, int64_t uv_stride,
                           const int64_t *a1, const int64_t *a2, const double *vis, double *grid);
/* do_imaging, :509-549, with imgfn = aw_imaging (:452-478): uvw in wavelengths; image and psf are N x N doubles
 * (required), pmax a HOST pointer (may be NULL).  Doweight order: weights from the MIRRORED uvw (:531-535), as for
 * every do_imaging kind.  The mirror negates u, v, w and conjugates vis; it does not swap a1 / a2 (:551-562).  The
 * image pass (wt * vis1) and the PSF pass (wt) share each batch's antenna pairs, keys, kernel table and binned
 * records: the table is built once per batch of 2^20 visibilities (read-only option "aw_tables_built"), where two
 * aw_imaging calls would build it twice.  Out-of-range antennas or w-bins are dropped and counted
 * (gridhip_last_dropped) as by gridhip_awgrid_dev.  The _dev form takes device-resident arrays and allocates nothing
 * after the first call of a shape; both forms synchronise (pmax). */
int gridhip_do_imaging_aw(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                          const double *wkerns, const double *wvals, const double *akerns, int64_t n,
                          const double *u, const double *v, const double *w, int64_t uv_stride,
                          const int64_t *a1, const int64_t *a2, const double *vis, double *image, double *psf,
                          double *pmax);
int gridhip_do_imaging_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                              int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                              int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                              const int64_t *a1, const int64_t *a2, const double *vis, double *image,
                              double *psf, double *pmax);
/* aw_gridding, src/ImageDataset.hs:54-77, as one call: uvw in METRES (uv_stride 3 for the /vis/uvw (n,3) matrix) and
 * f in Hz -> uvw_lambda (x f / 299792458, :181-187) -> doweight -> mirror_uvw -> aw_imaging of vis1 * wt ->
 * make_grid_hermitian -> real . ifft.  Doweight order: weights from the UN-mirrored uvw (:59-60), unlike do_imaging.
 * image (required) is N x N doubles, not normalised; imax (HOST pointer, may be NULL) is its maximum.  No PSF, as in
 * the reference.  The _dev form's only host round-trip is that scalar. */
int gridhip_aw_gridding(gridhip_ctx *ctx, double theta, int64_t lam, double f, int64_t W, int64_t Q, int64_t S,
                        int64_t A, const double *wkerns, const double *wvals, const double *akerns, int64_t n,
                        const double *u, const double *v, const double *w, int64_t uv_stride,
                        const int64_t *a1, const int64_t *a2, const double *vis, double *image, double *imax);
int gridhip_aw_gridding_dev(gridhip_ctx *ctx, double theta, int64_t lam, double f, int64_t W, int64_t Q, int64_t S,
                            int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                            int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                            const int64_t *a1, const int64_t *a2, const double *vis, double *image,
                            double *imax);
/* do_imaging, :509-549: mirror -> weight -> grid(vis*wt), grid(wt) -> hermitian -> ifft -> /max(psf).
 * kind: 0 simple_imaging; 1 conv_imaging (Q, gh, gw, kv); 2 w_cache_imaging (wstep, Q, npixFF, gh = npixKern).
 * image and psf are N x N doubles. */
int gridhip_do_imaging(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF,
                       int64_t gh, int64_t gw, const double *kv, double theta, int64_t lam, int64_t n,
                       const double *u, const double *v, const double *w, int64_t uv_stride,
                       const double *vis, double *image, double *psf, double *pmax);
/* The same with every array argument resident on the device (kv, u, v, w, vis in; image, psf out: ordinary device
 * allocations): nothing crosses PCIe, and after the first call of a shape nothing is allocated or freed (the scratch
 * comes from a pool the context keeps).  pmax stays a HOST pointer (may be NULL).  The call synchronises the stream
 * (the w-bin rule reads min / max back to the host exactly as the reference's nested CPU.run does, :430). */
int gridhip_do_imaging_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh,
                           int64_t gw, const double *kv, double theta, int64_t lam, int64_t n, const double *u,
                           const double *v, const double *w, int64_t uv_stride, const double *vis, double *image,
                           double *psf, double *pmax);
/* w_cache_imaging with device-resident u, v, w (wavelengths), vis and N x N grid (overwritten). */
int gridhip_w_cache_imaging_dev(gridhip_ctx *ctx, int64_t wstep, int64_t qpx, int64_t npixFF, int64_t npixKern,
                                double theta, int64_t lam, int64_t n, const double *u, const double *v,
                                const double *w, int64_t uv_stride, const double *vis, double *grid);

/* ---- prediction: a model image -> visibilities, the other half of a major cycle -------------------------------------
 * The model is a real N x N image, N = gridhip_image_size(theta, lam), row-major [y][x] and laid out as the `image` that
 * do_imaging returns.  u, v and w are taken exactly as the imaging function of that kind takes them: same units (uvw in
 * wavelengths), same uv_stride, no mirroring.  For each kind let A be the imaging function's linear map from visibilities
 * to the N x N grid.  Then
 *     F       = fft_c(model)   the centred forward transform, unnormalised (= gridhip_fft2_centered(.., inverse = 0) of
 *                              the model as complex)
 *     pred    = A^H F          the exact adjoint of the imaging function's scatter:
 *       simple   pred[k] = F[y_k, x_k], the nearest-cell rule of gridhip_grid (n is the grid HEIGHT for both axes); NaN
 *                or out-of-grid coordinates predict exactly 0
 *       conv     degrid2 with conj(kv), W = 1                        (conv_imaging grids with kv)
 *       w_cache  degrid2 with the UNconjugated w_kernel planes      (w_cache_imaging grids with their conjugates), on
 *                the w-bins of w_cache_imaging (the wstep rule)
 *       aw       awdegrid with conj(wkerns), conj(akerns)           (the identity stated at gridhip_awdegrid)
 *     vis_out = pred, or vis_sub - pred (the residual) when vis_sub != NULL.
 * The centred inverse transform's adjoint is N^-2 fft_c (odd N too), so for every kind, any vis and any real model
 *     sum(model * Re(ifft_c(imgfn(vis)))) == N^-2 Re(vdot(vis, predict(model)))
 * and this is the physically right prediction: a real sky's visibilities are its unnormalised DFT seen through the
 * unconjugated w / A kernels.
 * kind: 0 simple, 1 conv (Q, gh, gw, kv), 2 w_cache (wstep (<= 0: 2000), Q = qpx, npixFF, gh = npixKern; gw unused):
 * do_imaging's layout.  The host forms are synchronous; the _dev forms take device pointers (model, u, v, w, kv,
 * wkerns, wvals, akerns, a1, a2, vis_sub, vis_out) and are asynchronous on the context's stream, except kind 2, which
 * reads the w-bins' min and max back as gridhip_do_imaging_dev does.  vis_out is overwritten, never accumulated;
 * vis_out == vis_sub (an in-place residual) is allowed.  All arguments are checked before anything is touched: a refused
 * call (bad kind, NULL model, NULL vis_out with n > 0, bad shapes) returns GRIDHIP_EINVAL and leaves vis_out unchanged.
 * A support the gather cannot hold is GRIDHIP_EUNSUPPORTED, as for degrid2 and awdegrid.  Out-of-range antennas or aw
 * w-bins predict exactly 0 (vis_sub[k] in the residual form) and are counted by gridhip_last_dropped as the gather counts
 * them.  Scratch comes from the context's pool: after the first call of a shape a _dev call allocates nothing.  The
 * w_cache kind takes w_cache_imaging's cached kernel table as it is; that cache is keyed on the w range, so predicting
 * on un-mirrored w after a do_imaging (which mirrors) may rebuild it.  With timing enabled (gridhip_timing) ms_prepass
 * is the transform (head kernel + FFT) and ms_kernel the gather and the epilogue. */
int gridhip_predict(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                    const double *kv, double theta, int64_t lam, const double *model, int64_t n,
                    const double *u, const double *v, const double *w, int64_t uv_stride,
                    const double *vis_sub, double *vis_out);
int gridhip_predict_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                        const double *kv, double theta, int64_t lam, const double *model, int64_t n,
                        const double *u, const double *v, const double *w, int64_t uv_stride,
                        const double *vis_sub, double *vis_out);
/* aw: wkerns [W][Q][Q][S][S], wvals the W plane w-values searched by findClosest, akerns [A][S][S], as aw_imaging. */
int gridhip_predict_aw(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                       const double *wkerns, const double *wvals, const double *akerns, const double *model,
                       int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                       const int64_t *a1, const int64_t *a2, const double *vis_sub, double *vis_out);
int gridhip_predict_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                           const double *wkerns, const double *wvals, const double *akerns, const double *model,
                           int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                           const int64_t *a1, const int64_t *a2, const double *vis_sub, double *vis_out);

/* ---- imagers: bind the baselines once, one asynchronous call per major cycle (device pointers) ----------------------
 * A major cycle is
 *     residual = predict(model, vis_sub = vis);  image, psf, pmax = do_imaging(residual)
 * and in it uvw, the antenna pairs, the kernels, theta and lam never change: only model and, at most, vis do.  An imager
 * is created once from those and is DEFINED BY THE TWO CALLS IT REPLACES.  For the arguments given at creation, with
 * predict* / do_imaging* the _dev entry points of the imager's kind:
 *   cycle(model, vis)   image = the `image` output of do_imaging*(vis - predict*(model)); vis_res, when given,
 *                       = vis - predict*(model), un-mirrored and un-weighted as predict returns it (vis_res == vis: in place)
 *   cycle(NULL, vis)    image = the `image` output of do_imaging*(vis); vis_res, when given, receives vis
 *   psf, pmax           the `psf` / `pmax` outputs of do_imaging* for these baselines (they do not depend on vis)
 *   predict(model, vis_sub, vis_out)   gridhip_predict*_dev with the same arguments
 * which fixes every convention: weights from the mirrored uvw, a1 / a2 not swapped by the mirror, the image normalised by
 * pmax, prediction on the UN-mirrored baselines with the conjugated tables, dropped baselines predicting exactly 0 and
 * gridding nothing, NaN coordinates as the simple kind treats them.  Results agree with the two calls to the tolerance
 * the fp64 atomics of either side allow (1e-10 of the largest magnitude), not bit for bit.
 * Creation (may synchronise; the one place the w_cache kind reads a min / max back) slices and scales the strided uvw,
 * mirrors, histograms and applies the uniform weights, computes the w-bins of both streams, builds or copies the kernel
 * tables into memory of the imager's own, bins both record sets, grids the PSF and runs its tail.  Every creation input
 * may be freed or overwritten once it returns.  gridhip_last_dropped and gridhip_aw_last_stats then report the mirrored
 * stream's binning, "aw_tables_built" both streams' tables.  Everything is checked at creation by gridhip_predict's /
 * gridhip_aw_imaging's rules (GRIDHIP_EINVAL); a support the gather cannot hold, more than 65536 w-planes or a shape
 * outside the aw limits is GRIDHIP_EUNSUPPORTED.  A refused creation leaves *imager NULL and nothing allocated.
 * A cycle is: head kernel + forward FFT of the model, the gather over the un-mirrored records, ONE pass over the
 * visibilities (subtract, store vis_res, conjugate where mirrored, times the weight), the scatter over the mirrored
 * records, Hermitian fill + inverse FFT + real part divided by the stored pmax.  No PSF pass, no pre-pass, no table
 * build, no histogram.  cycle and predict enqueue on the context's stream and return: after the first cycle (which may
 * grow the context's launcher scratch) they allocate nothing, never synchronise, read nothing back and enqueue kernels
 * only - no memset node - so a cycle can be captured into a graph.  With timing enabled ms_prepass is the prediction
 * side (transform, gather, the pass over the visibilities) and ms_kernel the scatter and the tail.
 * The prediction gathers on the un-mirrored baselines and do_imaging scatters on the mirrored ones, and the two
 * binnings are not mirror images of each other bit for bit (floor(.5 + x), the w-bin rule and findClosest are not odd
 * functions): an imager keeps BOTH record sets, and for the aw kind both kernel tables ((wk, ak) keyed on the mirrored
 * stream, (conj wk, conj ak) on the un-mirrored one, per batch of 2^20 visibilities as gridhip_aw_plan holds them); for
 * w_cache one table per stream's w range (the gather's planes are the w_kernels, the scatter's their conjugates: two
 * tables even where the ranges agree).  Supports the tap-reusing kernel has no instantiation for go through
 * sub-footprints as they do for plans (their zero-padded table is rebuilt in the context's scratch by each pass).
 * Memory an imager holds: per visibility 8 B (the weight, its sign the mirror flag) + 16 B (the prediction, which the
 * pass over the visibilities turns into the gridder's input in place) + 2 x 8 B records (x P for sub-footprints), or
 * 4 x 8 B coordinates instead of records for the simple kind; per N^2 cell 16 B (grid) + 16 B (transform) + 8 B (psf),
 * and 16 B more for odd N; the kernel tables (conv: 2 tables; w_cache: one plane per w-bin of each stream; aw: each
 * batch's distinct kernels, twice) and one hipFFT plan; after its first clean or deconvolve also clean's state block and
 * tile table, 64 B + 16 B per 16 x 128 cells, after its first msclean that call's scratch (see there), and after its first restore without a `beam` output 64 B for the fitted beam;
 * with spectral terms (see "wide-band imaging") 8 B + 16 B more per visibility, 2T - 1 images and mfclean's scratch
 * (all released at destroy).
 * kind 0 simple, 1 conv, 2 w_cache: gridhip_do_imaging's / gridhip_predict's argument layout (w may be NULL for kinds 0
 * and 1).
 * kind 4 w-stacking (see "w-stacking"): wstep = the w step, Q = qpx, npixFF, gh = npixKern, gw = M (the planes per layer),
 * kv ignored; Q == 0: image-domain layers, npixFF the margin and gh the subgrid ("w-stacking", IMAGE-DOMAIN LAYERS: no
 * tables, and the image and the PSF are 0 outside the trusted region).  The two calls it replaces are gridhip_do_imaging_wstack_dev and gridhip_predict_wstack_dev, so its image
 * is 2 Re D(wt vis1) / pmax, not the Hermitian fill of kinds 0 to 2 ("DO_IMAGING WITH A STACK" explains the difference),
 * and its prediction is the stack's on the un-mirrored stream.  A visibility whose w is not finite grids nothing,
 * predicts exactly 0 and leaves vis_res[k] = vis[k]; n > 0 without any finite w gives what that call gives (a division by
 * pmax = 0).  Checked at creation by the stack's rules: wstep < 1, M < 1, the w-kernel shape rule (Q == 0: the subgrid and
 * margin rule) or w == NULL with n > 0
 * are GRIDHIP_EINVAL, more than 4096 layers on either stream, M > 65536, |w / wstep| > 2^52 or n >= 2^31 - 256
 * GRIDHIP_EUNSUPPORTED.  gridhip_do_imaging* and gridhip_predict* keep refusing kind 4 (they have their _wstack forms),
 * and kind 3 is refused here (aw has its own creation calls).  The imager holds a stack on each stream - the un-mirrored
 * one for the predict passes only, the mirrored one for the image passes only: v < 0 negates w, so plane ranges, pmin and
 * layer bounds differ - which share ONE kernel table K, one conj(K) and the imager's hipFFT plan, and have one N x N
 * complex grid each.  gridhip_last_dropped after creation reports the mirrored stack's total.  A cycle is: per layer of
 * the un-mirrored stack head kernel + forward FFT + gather; ONE pass over the visibilities in the mirrored stack's layer
 * order (option "wstack_middle"); per layer of the mirrored stack scatter + inverse FFT + screen; one division by the
 * stored pmax.  predict, selfcal, peel, flag and the wide-band calls take the stream-order passes.  Memory of this kind:
 * per visibility 8 B (the weight) + 16 B (the prediction in stream order) + two 16 B layer-ordered blocks + three 4 B
 * indices (each stack's and their composition) + 2 x 24 B of layer-ordered coordinates and bins, and the layers'
 * records; per N^2 cell 2 x 16 B (the two grids) + 8 B (psf); 2 x M Q^2 S^2 x 16 B of tables and one hipFFT plan.
 * n = 0 is a valid imager whose image is zero.  cycle with NULL vis or image (n > 0) is GRIDHIP_EINVAL and
 * touches nothing.  An imager belongs to its context (same device, same stream, not thread-safe) and must be destroyed
 * before it; any other call on the context between two imager calls - do_imaging or predict of another shape, another
 * imager, a rebuild of the w-kernel cache - leaves its results unchanged. */
typedef struct gridhip_imager gridhip_imager;
int gridhip_imager_create_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh,
                              int64_t gw, const double *kv, double theta, int64_t lam, int64_t n, const double *u,
                              const double *v, const double *w, int64_t uv_stride, gridhip_imager **imager);
/* aw: gridhip_do_imaging_aw's / gridhip_predict_aw's argument layout */
int gridhip_imager_create_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                                 int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                                 int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                                 const int64_t *a1, const int64_t *a2, gridhip_imager **imager);
/* the PSF (N x N doubles on the device, copied on the stream) and its maximum (a HOST pointer), both computed at
 * creation; either may be NULL */
int gridhip_imager_psf_dev(gridhip_imager *imager, double *psf, double *pmax);
/* one major-cycle step.  model NULL: no prediction.  vis_res NULL: the residual visibilities are not returned */
int gridhip_imager_cycle_dev(gridhip_imager *imager, const double *model, const double *vis, double *image,
                             double *vis_res);
/* the prediction alone, gridhip_predict's vis_sub / vis_out rules */
int gridhip_imager_predict_dev(gridhip_imager *imager, const double *model, const double *vis_sub, double *vis_out);
int gridhip_imager_destroy(gridhip_imager *imager);

/* ---- deconvolution: Hogbom CLEAN on the device, the minor cycle between two major cycles ------------------------------
 * The reference has no deconvolution: the semantics are defined here.  psf, residual and model are real N x N images,
 * row-major [y][x], laid out as do_imaging's `image` and `psf`.  The PSF's zero-lag cell is c = (N / 2, N / 2) in integer
 * division, for even and odd N: where gridhip_fft2_centered(inverse = 1) puts it, and where an imager's PSF has its
 * maximum.
 *     repeat at most niter times:
 *         k = the flat index y * N + x with the largest |residual[k]| over the cells border <= y, x < N - border;
 *             ties go to the lowest flat index; a NaN cell is never selected
 *         p = residual[k]
 *         if |p| <= threshold: stop                            (tested before anything is subtracted)
 *         f = gain * p                                         (rounded once)
 *         model[k] += f
 *         residual[y', x'] -= f * psf[y' - y + c, x' - x + c]  for every cell whose PSF index lies in the grid and, when
 *                                                              patch > 0, within |y' - y| <= patch and |x' - x| <= patch
 *     stats = { iterations performed, residual[k*] (signed), k* as a double, sum of all f added }
 *             where k* is the peak of the final residual under the same search rule
 * The product f * psf is rounded before it is subtracted (no fused multiply-add), every comparison is (|value|, lower
 * index wins) and nothing is accumulated with atomics: a call is deterministic, bit for bit, whatever the scheduling,
 * and the host, _dev and imager forms give the same bits.  residual is updated in place.  model is accumulated into,
 * never zeroed (model = model + clean(...) is one call on the same model).  stats is four doubles, written on the
 * device (a host array for gridhip_clean); it may be NULL.  niter = 0 is valid: it changes nothing and reports the
 * current peak.  If no cell can be selected (every searched cell is NaN) the loop stops and stats reports a NaN peak at
 * index -1.  All arguments are checked before anything is touched, GRIDHIP_EINVAL: N >= 1, 0 < gain <= 1,
 * threshold >= 0, niter >= 0, 0 <= border, 2 * border < N, patch >= 0, non-NULL psf, residual and model, no two of the
 * three arrays overlapping (nmajor >= 0 and, for an imager with visibilities, non-NULL vis for deconvolve).  N above
 * 1048560 is GRIDHIP_EUNSUPPORTED.
 * The image is cut into tiles of 16 rows x 128 columns and a device table keeps each tile's peak; it is built by one pass
 * over the residual per call.  An iteration is two kernels: one subtracts the shifted, scaled PSF from the tiles the PSF
 * (or the patch) overlaps - it is launched over those tiles only - and recomputes their table entries in the same pass;
 * a one-work-group kernel reduces the table to the next peak, tests the stop rule and takes the next component.  With
 * patch > 0 an iteration costs the patch area plus the table, not N^2.  The stop condition lives on the device: niter
 * iterations are enqueued unconditionally, and a launch whose state is stopped or out of iterations returns at its first
 * instruction.  gridhip_clean is synchronous and stages host arrays through the context's pool.  The _dev forms take
 * device pointers, enqueue kernels only on the context's stream (2 + 2 * niter launches; no memset or copy node),
 * allocate nothing after the first call of a shape, never synchronise and read nothing back, so they can be captured
 * into a graph like an imager's cycle.  Scratch (64 B + 16 B per tile) comes from the context's pool, or for the imager
 * forms from memory the imager owns. */
int gridhip_clean(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                  double threshold, int64_t niter, int64_t border, int64_t patch, double *stats);
int gridhip_clean_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                      double threshold, int64_t niter, int64_t border, int64_t patch, double *stats);
/* gridhip_clean_dev with the imager's own PSF (nothing is copied) and N */
int gridhip_imager_clean_dev(gridhip_imager *imager, double *residual, double *model, double gain, double threshold,
                             int64_t niter, int64_t border, int64_t patch, double *stats);
/* visibilities -> model image in one call, DEFINED BY THE CALLS IT REPLACES:
 *     repeat nmajor times: image = cycle(model, vis); clean(image, model) with stats + 4 * i (when stats != NULL)
 *     image = cycle(model, vis)
 * so that on return image is do_imaging(vis - predict(model))'s image for the returned model.  model is the caller's
 * and must be initialised (zeros for a fresh start); stats is nmajor x 4 doubles on the device, or NULL.  Asynchronous,
 * allocation-free after the first call and capturable, as cycle and clean are. */
int gridhip_imager_deconvolve_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                  int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                  int64_t patch, double *stats);

/* ---- multi-scale deconvolution: multi-scale CLEAN (Cornwell 2008) on the device, beside the Hogbom one -------------------
 * Hogbom CLEAN takes one cell per component, so extended emission costs thousands of components and leaves a pedestal.
 * Here a component is a tapered paraboloid of one of S scales.  The reference has neither form: the semantics are defined
 * here.  psf, residual and model are as for gridhip_clean, c = N / 2.  scales a_0 < a_1 < ... < a_{S-1} are in cells
 * (doubles), 1 <= S <= 6, a_0 == 0, a_{S-1} <= 32; bias b_s is finite and > 0, one per scale.  scales and bias are HOST
 * arrays for every form: they fix launch shapes and kernel arguments and are read at call time.
 * SCALE KERNEL: m_0 is the delta.  For s >= 1, R_s = ceil(a_s) - 1 and
 *     t(dy, dx) = max(0, 1 - (dx^2 + dy^2) / a_s^2)   over |dy|, |dx| <= R_s
 * in fp64, the quotient rounded, no fused multiply-add; sum = its taps added from +0.0, each row in dx order, then the rows
 * in dy order; m_s = t / sum.  m_s is made on the device by a kernel (nothing is uploaded).
 * CONVOLUTION: (m (*) X)[y, x] = sum of X[y - dy, x - dx] * m(dy, dx), cells outside the image counting as zero, the taps
 * dy ascending, then dx ascending, one fused multiply-add each from +0.0 (the restore's rule).  Convolving with the delta
 * is the identity and is not computed: P_00 is psf itself and R_0 is residual itself, in place.
 * SET-UP:  P_s = m_s (*) psf;  P_st = m_t (*) P_s for s <= t (P_ts means P_st);  R_t = m_t (*) residual for t >= 1;
 *          q_s = P_ss[c, c].
 *     repeat at most niter times:
 *         for each scale: k_s = the peak of |R_s| under clean's search rule (border, ties to the lowest flat index, NaN
 *                         never), p_s = R_s[k_s]
 *         stop if no cell of R_0 can be selected or |p_0| <= threshold   (before anything is subtracted; the threshold is
 *                                                                         in units of the plain residual)
 *         s* = the scale with the largest |b_s * (p_s / q_s)|  (the quotient rounded, then the product; ties to the lowest
 *              s; a scale whose q_s is not positive and finite, or which has no selectable cell, never wins - if none
 *              can, the loop stops)
 *         f = gain * (p_s* / q_s*),  k = k_s* = (y, x)
 *         model[y', x'] += f * m_s*(y' - y, x' - x)         over the kernel's support, clipped to the image; the product
 *                                                           is rounded, then added (the delta's one cell receives
 *                                                           gain * (p / q) in one fused step, as gridhip_clean's does)
 *         R_t[y', x'] -= f * P_{s* t}[y' - y + c, x' - x + c]   for every t; the clipping and the patch rule are exactly
 *                                                           gridhip_clean's; the product is rounded, then subtracted
 *     stats = 12 doubles { iterations, final p_0, final k_0, the s* of the last component taken (-1 if none), sum of f, 0,
 *                          n_0 .. n_5 }, n_s the number of components taken at scale s
 * No atomics anywhere: a call is deterministic bit for bit, and the host, _dev and imager forms give the same bits.  With
 * S = 1, scales = {0}, bias = {1} and psf[c, c] == 1.0, residual and model come out with the bits of gridhip_clean.
 * Only residual (R_0) and model are returned; the smoothed residuals are scratch.
 * Arguments: gridhip_clean's rules, and GRIDHIP_EINVAL for S out of range, NULL scales or bias, scales not strictly
 * increasing or a_0 != 0, a bias not finite and positive - all checked before anything is touched; a_{S-1} > 32 is
 * GRIDHIP_EUNSUPPORTED (it would need an FFT-based set-up).
 * The set-up convolutions are LDS-tiled direct convolutions (the restore's tile and halo staging, the taps staged once per
 * work-group; a work-group whose staged window holds no non-zero cell stores +0.0, the sum's own bits).  An iteration is
 * two launches as gridhip_clean's: one covers the tiles the update region overlaps times S - slice t subtracts
 * f * P_{s* t} from R_t and recomputes the entries of table t in the same pass - and a one-work-group kernel reduces the S
 * tables, applies the stop test and the scale choice and adds the model blob (at most 63 x 63 cells).  The stop condition
 * lives on the device; a launch that finds the state stopped returns at its first instruction.
 * gridhip_msclean is synchronous and stages host arrays through the context's pool.  The _dev forms enqueue kernels only on
 * the context's stream (no memset or copy node), allocate nothing after the first call of a shape, read nothing back and
 * never synchronise.  Scratch is S - 1 smoothed residuals, S (S + 1) / 2 - 1 cross-PSFs (N x N doubles each), the taps,
 * the state block and S tile tables: from the context's pool, or, for the imager forms, memory the imager owns (grown -
 * one hipFree - by a call with a longer scale list).  An imager keeps the taps and the cross-PSFs between calls, keyed by
 * the scale list: its PSF never changes, so they are built by the first call with a given list only. */
int gridhip_msclean(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                    const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                    int64_t patch, double *stats);
int gridhip_msclean_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                        const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                        int64_t border, int64_t patch, double *stats);
/* gridhip_msclean_dev with the imager's own PSF (nothing is copied) and N */
int gridhip_imager_msclean_dev(gridhip_imager *imager, double *residual, double *model, int64_t S, const double *scales,
                               const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                               int64_t patch, double *stats);
/* gridhip_imager_deconvolve_dev with the multi-scale minor cycle, DEFINED BY THE CALLS IT REPLACES:
 *     repeat nmajor times: image = cycle(model, vis); msclean(image, model) with stats + 12 * i (when stats != NULL)
 *     image = cycle(model, vis)
 * stats is nmajor x 12 doubles on the device, or NULL.  The cross-PSFs are built by the first of the nmajor cleans. */
int gridhip_imager_msdeconvolve_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                    int64_t nmajor, int64_t S, const double *scales, const double *bias, double gain,
                                    double threshold, int64_t niter, int64_t border, int64_t patch, double *stats);

/* ---- image statistics: a robust noise estimate of a map, on the device -----------------------------------------------
 * The reference has none of this: the semantics are defined here.  image is a real N x N image, row-major; mask is
 * N x N bytes, or NULL for none; border follows clean's rule.  A cell k = y * N + x TAKES PART when
 *     border <= y, x < N - border,   mask == NULL or mask[k] != 0,   and image[k] is finite (NaN and +-Inf never).
 * Let n be the number of such cells.  They are ORDERED by the usual order-preserving 64-bit key of a double: all bits
 * of a negative value flipped, the sign bit of a non-negative value flipped, the keys compared as unsigned integers.
 * This puts -0.0 before +0.0 and needs no comparison of doubles.
 *     median = the element of rank (n - 1) / 2 (integer division: the LOWER median; an element of the image, never an
 *              average)
 *     d_k    = |image[k] - median|, the difference rounded once, over the same cells
 *     MAD    = the lower median of the d_k
 *     sigma  = 1.4826 * MAD, rounded once
 *     stats  = 8 doubles { n, median, MAD, sigma, min, max, the number of non-finite cells inside border and mask, 0 }
 *              (min and max under the key order; n = 0: median, MAD, sigma, min and max are NaN)
 * Every value is an order statistic or a count: the result is the same bits for the host, _dev and imager forms, for
 * two runs, and for a sort of the keys on the host.
 * Arguments, checked before anything is touched: GRIDHIP_EINVAL for N < 1, border < 0 or 2 * border >= N, NULL image
 * or stats, mask overlapping image, stats overlapping image or mask; N above 1048560 is GRIDHIP_EUNSUPPORTED.
 * The implementation is a radix select on the key, never a sort: one pass over the image builds the histogram of one
 * 13-bit digit over the cells whose higher digits equal the prefix chosen so far (each work-group into LDS with 32-bit
 * integer atomics, then its non-zero bins into a 64-bit table with integer atomics), a one-work-group kernel takes
 * the digit that holds the wanted rank; 5 passes give the median, 5 more over d_k the MAD.  The first pass also
 * takes n, min, max and the skipped count.  There is no floating-point atomic and no sum of doubles.  21 launches
 * whatever the image holds.  (Context option "noise_bits" = 8 selects 8-bit digits, 8 + 8 passes, for comparison.)
 * gridhip_image_stats is synchronous and stages host arrays through the context's pool.  The _dev and imager forms
 * enqueue kernels only on the context's stream (the tables are zeroed by a kernel: no memset or copy node), allocate
 * nothing after the first call, read nothing back and never synchronise: they can be captured.  Scratch (about 80 KB)
 * comes from the context's pool, or for the imager form from memory the imager owns; stats is on the device. */
int gridhip_image_stats(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                        double *stats);
int gridhip_image_stats_dev(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                            double *stats);
/* gridhip_image_stats_dev with the imager's N and its own scratch */
int gridhip_imager_image_stats_dev(gridhip_imager *imager, const double *image, const uint8_t *mask, int64_t border,
                                   double *stats);

/* ---- masks and noise-based stop levels: the _auto forms of clean and msclean --------------------------------------------
 * Everything is gridhip_clean's / gridhip_msclean's, with two additions.
 * MASK: N x N bytes, or NULL for none.  A cell with mask[k] == 0 is never selected: it is skipped in the search exactly
 * as a NaN cell is - for msclean in the search of every scale, so the mask constrains component CENTRES.  Nothing else
 * changes: the PSF is subtracted over the whole update region, masked or not, a multi-scale blob may extend over
 * masked-out cells, and the final peak and index of stats are the peak UNDER THE MASK.  The mask must not overlap
 * residual or model (GRIDHIP_EINVAL).
 * STOP LEVEL: noise points to ONE double, sigma - on the device for the _dev and imager forms, on the host for the host
 * forms - so that element 3 of a gridhip_image_stats result can be passed as it is.  p1 is the first peak the call
 * finds, before anything is subtracted (for msclean p_0, the plain residual's peak).
 *     T = max(threshold, nsigma * sigma, peak_frac * |p1|)     each product rounded once
 * computed once per call, on the device, and the loop's test is |p| <= T where it was |p| <= threshold.  nsigma == 0
 * leaves its term out, and noise may then be NULL; peak_frac == 0 leaves its term out; so does a p1 that does not exist
 * (nothing selectable).  If nsigma > 0 and sigma is NaN the call stops at once and touches nothing but stats (reason 3):
 * it does not fall back to a threshold the caller did not ask for.  GRIDHIP_EINVAL before anything is touched: nsigma
 * not finite or < 0, peak_frac outside [0, 1) or NaN, nsigma > 0 with NULL noise.
 * STATS: clean writes 8 doubles, the 4 of gridhip_clean then { T, reason, p1, 0 }; msclean 16, the 12 of gridhip_msclean
 * then the same four.  reason, the first of these that holds when the loop stops:
 *     3  no usable sigma            2  nothing selectable (for msclean also: no scale can be chosen)
 *     1  |peak| <= T                0  niter components taken
 * (Rounding, for a restatement that wants the bits: gridhip_clean's model cell and its flux receive gain * p in one fused
 * multiply-add each; f itself, which scales the PSF, is the rounded product.  gridhip_msclean fuses the delta's cell only.)
 * IDENTITY: with mask == NULL, nsigma == 0 and peak_frac == 0, residual, model and the first 4 (12) stats have the bits
 * of gridhip_clean (gridhip_msclean).  Launch counts, scratch and capturability are those of the plain forms; a lane of
 * the tile kernel reads the two mask bytes of its two-cell slot, and the kernels without a mask are the code they were. */
int gridhip_clean_auto(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                       double threshold, int64_t niter, int64_t border, int64_t patch, const uint8_t *mask, double nsigma,
                       const double *noise, double peak_frac, double *stats);
int gridhip_clean_auto_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                           double threshold, int64_t niter, int64_t border, int64_t patch, const uint8_t *mask,
                           double nsigma, const double *noise, double peak_frac, double *stats);
int gridhip_msclean_auto(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                         const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                         int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                         double peak_frac, double *stats);
int gridhip_msclean_auto_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                             const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                             int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                             double peak_frac, double *stats);
/* the _auto_dev forms with the imager's own PSF and N */
int gridhip_imager_clean_auto_dev(gridhip_imager *imager, double *residual, double *model, double gain, double threshold,
                                  int64_t niter, int64_t border, int64_t patch, const uint8_t *mask, double nsigma,
                                  const double *noise, double peak_frac, double *stats);
int gridhip_imager_msclean_auto_dev(gridhip_imager *imager, double *residual, double *model, int64_t S,
                                    const double *scales, const double *bias, double gain, double threshold,
                                    int64_t niter, int64_t border, int64_t patch, const uint8_t *mask, double nsigma,
                                    const double *noise, double peak_frac, double *stats);
/* visibilities -> model image with minor cycles that know the noise, DEFINED BY THE CALLS IT REPLACES:
 *     repeat nmajor times (i = 0 ..):
 *         image = cycle(model, vis)
 *         image_stats(image, NULL, border) -> istats + 8 i     (the whole search region; the clean mask is NOT applied:
 *                                                               sigma of the map)
 *         clean_auto | msclean_auto(image, model, ..., mask, nsigma, noise = &istats[8 i + 3], peak_frac)
 *                                                            -> stats + 8 i | stats + 16 i   (when stats != NULL)
 *     image = cycle(model, vis)
 * istats is nmajor x 8 doubles on the device; when it is NULL the imager keeps the 8 doubles itself.  Asynchronous,
 * allocation-free after the first call and capturable.  All nmajor cycles are enqueued and run: a major cycle whose
 * clean stops at once still images and measures; nothing on the device skips a cycle. */
int gridhip_imager_deconvolve_auto_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                       int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                       int64_t patch, const uint8_t *mask, double nsigma, double peak_frac,
                                       double *stats, double *istats);
int gridhip_imager_msdeconvolve_auto_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                         int64_t nmajor, int64_t S, const double *scales, const double *bias, double gain,
                                         double threshold, int64_t niter, int64_t border, int64_t patch,
                                         const uint8_t *mask, double nsigma, double peak_frac, double *stats,
                                         double *istats);

/* ---- auto-masking: the clean mask of a major cycle from the map it is about to clean, on the device ------------------------
 * The reference has no masks at all: the semantics are defined here.  image is a real N x N image, row-major, k = y * N +
 * x; mask is N x N bytes, UPDATED IN PLACE; border follows clean's rule.  A cell TAKES PART when
 *     border <= y, x < N - border   and image[k] is finite (NaN and +-Inf never):
 * gridhip_image_stats' rule without a mask.  v(k) = image[k], or |image[k]| when absolute != 0.
 * LEVELS.  noise points to ONE double, sigma - on the device for the _dev and imager forms, on the host for the host form -
 * so that element 3 of a gridhip_image_stats result can be passed as it is.  P is the maximum of v over the cells that
 * take part (under image_stats' key order: +0.0 above -0.0).
 *     T_hi = max(thr_hi, nsigma_hi * sigma, peak_frac * P)     each product rounded once
 *     T_lo = max(thr_lo, nsigma_lo * sigma, peak_frac * P)
 * A zero nsigma leaves its term out, and noise may be NULL when both are zero; a zero peak_frac leaves its term out.
 * STEPS.  Connectivity is 8 everywhere.
 *     1  H = { k takes part : v(k) > T_hi },  L = { k takes part : v(k) > T_lo }.  The comparison is strict: these are the
 *        cells clean's |p| <= T test would not stop at.  H is a subset of L.
 *     2  PRUNE.  The components of H are labelled; one with fewer than min_cells cells is dropped.  The seeds S are the
 *        cells of the components that survive.
 *     3  HYSTERESIS.  The components of L are labelled; one is kept if and only if it holds at least one cell of S.  K is
 *        the union of the kept components.
 *     4  GROW.  G = { k inside the border region : some cell of K lies within Chebyshev distance grow }.  grow is a host
 *        argument (it fixes the launch shape).  A non-finite cell inside the region may be in G; nothing outside the border
 *        region is ever set.
 *     5  ACCUMULATE.  A cell with mask[k] != 0 keeps its byte; a cell of G with mask[k] == 0 becomes 1.  No bit is ever
 *        cleared: a mask of zeros starts a run, and a caller's own regions are kept.
 * A component's label is the smallest k in it, which makes every intermediate result unique: the whole result is a
 * function of the input alone - the same bytes for the host, _dev and imager forms, for two runs, and for a flood fill on
 * the host.
 * stats is 8 doubles { T_hi, T_lo, P, components of H, of them surviving the prune, components of L kept, cells newly set,
 * reason }, all exact counts or once-rounded products.  reason is 0 when the steps ran.  Otherwise the mask is left exactly
 * as it was and the four counts are 0 - the first of these that holds:
 *     3  an nsigma term is wanted and sigma is NaN: T_hi and T_lo are NaN, P is the maximum (NaN without one)
 *     2  no cell takes part: P is NaN, and T_hi, T_lo are the levels without the peak_frac term
 * Arguments, checked before anything is touched.  GRIDHIP_EINVAL: thr_lo > thr_hi or nsigma_lo > nsigma_hi; thr or nsigma
 * negative or not finite; peak_frac outside [0, 1) or NaN; nsigma_hi > 0 with NULL noise; min_cells < 1; grow < 0; a NULL
 * image, mask or stats; mask or stats overlapping image, or each other; N < 1; border < 0 or 2 * border >= N.  Then
 * GRIDHIP_EUNSUPPORTED: grow > 32, or N > 46340 (labels are 32-bit cell indices).
 * The labelling is a union-find with a fixed pass structure, never a propagation repeated until nothing changes: a
 * work-group labels one 32 x 32 tile in LDS (each cell starts at the first cell of its horizontal run, runs are united
 * with the row above by 32-bit atomicMin on roots); a second kernel unites cells across tile edges and across the corners
 * where four tiles meet, in global memory; a third flattens.  label[k] <= k holds at every instant - a link always goes
 * from the larger root to the smaller - which bounds every loop by the index it starts from, whatever other threads do.
 * Component sizes are integer counts, taken per tile in LDS and added to the root once per (tile, component).  Growing is
 * one LDS-tiled kernel with a halo of grow cells.  There is no floating-point atomic: levels are compared, never summed.
 * gridhip_automask is synchronous and stages host arrays through the context's pool.  The _dev and imager forms enqueue
 * kernels only on the context's stream - 13 launches whatever the image holds, no memset or copy node - allocate nothing
 * after the first call, read nothing back and never synchronise: they can be captured.  Scratch (two int32 planes and a
 * byte plane, 9 bytes per cell) comes from the context's pool, or for the imager forms from memory the imager owns; stats
 * is on the device. */
int gridhip_automask(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                     double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                     double peak_frac, int64_t min_cells, int64_t grow, double *stats);
int gridhip_automask_dev(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                         double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                         double peak_frac, int64_t min_cells, int64_t grow, double *stats);
/* gridhip_automask_dev with the imager's N and its own scratch */
int gridhip_imager_automask_dev(gridhip_imager *imager, const double *image, uint8_t *mask, int64_t border, int absolute,
                                double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                                double peak_frac, int64_t min_cells, int64_t grow, double *stats);
/* visibilities -> model image under a mask that every major cycle extends itself, DEFINED BY THE CALLS IT REPLACES:
 *     repeat nmajor times (i = 0 ..):
 *         image = cycle(model, vis)
 *         image_stats(image, NULL, border)                                -> istats + 8 i
 *         automask(image, mask, border, absolute .. grow, noise = &istats[8 i + 3])   -> astats + 8 i
 *         clean_auto | msclean_auto(image, model, ..., mask, nsigma, noise = &istats[8 i + 3], peak_frac_clean)
 *                                                                         -> stats + 8 i | stats + 16 i   (when stats != NULL)
 *     image = cycle(model, vis)
 * mask is the caller's device buffer and may not be NULL: its content on entry is the starting mask, on return it holds
 * the accumulated mask.  A cycle whose mask is still empty cleans nothing (clean_auto's reason 2) and still images and
 * measures; nothing on the device skips a cycle.  istats and astats are nmajor x 8 doubles on the device; where one is NULL
 * the imager keeps the 8 doubles itself.  Every argument rule of the calls replaced is checked before anything is
 * enqueued.  Asynchronous, allocation-free after the first call and capturable. */
int gridhip_imager_deconvolve_automask_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                           int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                           int64_t patch, uint8_t *mask, double nsigma, double peak_frac_clean,
                                           int absolute, double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo,
                                           double peak_frac, int64_t min_cells, int64_t grow, double *stats,
                                           double *istats, double *astats);
int gridhip_imager_msdeconvolve_automask_dev(gridhip_imager *imager, const double *vis, double *model, double *image,
                                             int64_t nmajor, int64_t S, const double *scales, const double *bias,
                                             double gain, double threshold, int64_t niter, int64_t border, int64_t patch,
                                             uint8_t *mask, double nsigma, double peak_frac_clean, int absolute,
                                             double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo,
                                             double peak_frac, int64_t min_cells, int64_t grow, double *stats,
                                             double *istats, double *astats);

/* ---- local background and noise maps: a windowed median and MAD on a mesh, interpolated onto the image, on the device ------
 * The reference has none of this: the semantics are defined here.  gridhip_image_stats gives one sigma for a whole map;
 * the noise of a primary-beam-corrected image or a mosaic rises toward its edge, and it is several times higher around a
 * bright source.  This gives a sigma per cell.  image is a real N x N image, row-major, k = y * N + x; mask is N x N bytes,
 * or NULL for none.  A cell TAKES PART when
 *     border <= y, x < N - border,   image[k] is finite,   and   mask == NULL,  or  exclude == 0 and mask[k] != 0
 *     (gridhip_image_stats' rule),  or  exclude == 1 and mask[k] == 0  (the sources of a clean mask stay out of their own
 *     noise estimate).
 * MESH.  M = N - 2 * border, G = max(1, M / step) in integer division (gridhip_noise_map_nodes returns it).  Node i has
 * the centre c_i = border + min(i * step + step / 2, M - 1); node (i, j) owns the window |y - c_i| <= half, |x - c_j| <=
 * half, clipped to the border region.
 * NODE STATISTIC.  V is the window's cells that take part, ordered by gridhip_image_stats' 64-bit key.  For rounds r = 0, 1 ..
 *     1  med = the lower median of V (rank (n - 1) / 2)
 *     2  d_k = |v_k - med|, the difference rounded once
 *     3  MAD = the lower median of the d_k
 *     4  if r == nclip, or V is empty: stop
 *     5  L = kappa * (1.4826 * MAD), both products rounded once
 *     6  the cells with d_k > L leave V
 *     7  if none left: stop; else r += 1
 * With n_used the size of the final V and `rounds` the final r (the rounds that dropped a cell):
 *     nodes[4][G][G] = { background, rms, n_used, rounds }
 *     background = med if n_used >= min_count, else NaN;   rms = 1.4826 * MAD if n_used >= min_count and MAD > 0, else NaN
 * so a constant patch has a background and no rms.
 * MAPS, for a cell inside the border region.  i = the largest node with c_i <= y, or 0 when y < c_0; i1 = min(i + 1, G - 1);
 * fy = 0 when i1 == i or y < c_i, else (double)(y - c_i) / (double)(c_i1 - c_i); j, j1, fx the same from x.
 *     lerp(a, b, f) = a + f * (b - a) when both are finite - difference, product and sum each rounded, nothing fused -
 *                     a when only a is finite, b when only b is, NaN when neither is
 *     value = lerp(lerp(t[i][j], t[i][j1], fx), lerp(t[i1][j], t[i1][j1], fx), fy)
 * for t the background table and for t the rms table.  A cell outside the border region is NaN in both maps and in out.
 * out, by mode: 0 nothing; 1 image - background; 2 (image - background) / rms, a subtraction and then an IEEE division.  A
 * non-finite image cell propagates as the arithmetic gives it.
 * stats is 8 doubles { G, nodes with a background, nodes with an rms, the smallest rms of a node, the largest (both under
 * the key order; NaN when no node has one), the cells of out inside the region that are not finite (0 for mode 0), the
 * largest `rounds` of a node, 0 }.
 * Everything is an order statistic, a count or a fixed sequence of rounded operations: the same bits for the host and _dev
 * forms, for two runs, for a replayed graph, and for a restatement with a sort on the host.
 * Arguments, checked before anything is touched.  GRIDHIP_EINVAL: N < 1; border < 0 or 2 * border >= N; step < 1; half < 1;
 * kappa not finite or <= 0; nclip outside 0 .. 8; min_count < 1; exclude not 0 or 1; mode not 0, 1 or 2; a NULL image or
 * stats; a NULL out with mode != 0; any of nodes, background, rms, out and stats overlapping image, mask or each other -
 * but out may be image itself.  nodes, background, rms and (mode 0) out may each be NULL.  Then GRIDHIP_EUNSUPPORTED:
 * half > 64, or N > 1048560.  gridhip_noise_map_nodes returns GRIDHIP_EINVAL for the first three rules.
 * The node kernel is one work-group per node: the window's keys go into LDS once - (2 half + 1)^2 x 8 B, 133,128 B at
 * half = 64, which fits the 160 KB a work-group may take on gfx950 and not 64 KB - and every select of every round is a
 * radix select with 8-bit digits out of that copy, the MAD's over d_k recomputed from the keys; a cell that leaves V is
 * overwritten by a key no finite value has.  The histograms use 32-bit integer LDS atomics (context option
 * "noisemap_hist" chooses how, the same bits each way); there is no floating-point atomic and no sum of doubles.  A second
 * kernel writes the maps and out in one pass, a third the stats.
 * gridhip_noise_map is synchronous and stages host arrays through the context's pool.  The _dev form enqueues these three
 * kernels on the context's stream, whatever the image holds - no memset or copy node - allocates nothing after the first
 * call of a shape, reads nothing back and never synchronises: it can be captured.  Scratch (64 B, and the node table when
 * nodes is NULL) comes from the context's pool; stats is on the device. */
int64_t gridhip_noise_map_nodes(int64_t N, int64_t border, int64_t step);
int gridhip_noise_map(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int exclude, int64_t border,
                      int64_t step, int64_t half, double kappa, int64_t nclip, int64_t min_count, int mode, double *nodes,
                      double *background, double *rms, double *out, double *stats);
int gridhip_noise_map_dev(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int exclude,
                          int64_t border, int64_t step, int64_t half, double kappa, int64_t nclip, int64_t min_count,
                          int mode, double *nodes, double *background, double *rms, double *out, double *stats);

/* ---- restoring beam and restore: from clean's model and residual to a map, on the device -----------------------------
 * The reference stops at the dirty image: the semantics are defined here.  All images are real N x N, row-major [y][x];
 * the PSF's zero-lag cell is c = (N / 2, N / 2) in integer division, as for clean.
 * BEAM FIT: an elliptical Gaussian fitted to the main lobe of the PSF.  window >= 1 and 0 < cut < 1 are the caller's.
 *     R = min(window, c, N - 1 - c)
 *     p(dy, dx) = psf[c + dy, c + dx] / psf[c, c]
 *     a cell (dy, dx) != (0, 0) with |dy|, |dx| <= R takes part if and only if p <= 1 and
 *         p >= cut, or max(|dy|, |dx|) == 1 and p > 0
 *     (the second case lets the eight neighbours of the centre take part whenever their logarithm exists, so that a beam
 *     narrower than a couple of cells - what a uniformly weighted imager makes - is still fitted; a NaN cell never
 *     takes part)
 *     minimise  sum p^2 (A dx^2 + 2 B dx dy + C dy^2 + ln p)^2  over the participating cells
 * With w = p^2, a = dx^2, b = 2 dx dy, c = dy^2 (exact integers) and l = ln p, the nine sums of the normal equations
 *     M = [[sum (w a) a, sum (w a) b, sum (w a) c], [., sum (w b) b, sum (w b) c], [., ., sum (w c) c]] (symmetric),
 *     g = [sum (w a) l, sum (w b) l, sum (w c) l]
 * are accumulated in fp64 without fused multiply-adds and without atomics: each row dy in dx order from +0.0, then the rows
 * in dy order from +0.0.  M (A, B, C)^T = -g is solved by Cramer's rule (cofactor expansion along the first row).
 *     beam(dy, dx) = exp(-(A dx^2 + 2 B dx dy + C dy^2)), peak 1
 *     result = 8 doubles { A, B, C, bmaj, bmin, bpa, ncells, ok }
 * bmaj >= bmin are the FWHMs in cells, 2 sqrt(ln 2 / lambda) for the two eigenvalues (A + C) / 2 -+ sqrt(((A - C) / 2)^2
 * + B^2) of [[A, B], [B, C]] (a cell is theta / N radians); bpa is the direction of the major axis, the angle from +x
 * towards +y in radians, in (-pi/2, pi/2], 0 when A == C and B == 0; ncells is the number of participating cells.  The
 * fit FAILS when fewer than 3 cells take part, when det M is not positive, when psf[c, c] is not positive or not finite,
 * or when the fitted form is not positive definite (A > 0, C > 0, A C - B^2 > 0): it then writes ok = 0, the true
 * ncells and NaN in the other six.  A call is deterministic bit for bit.
 * RESTORE: 1 <= support <= 32 is a host argument (it fixes the launch shape, so that the call can be captured).
 *     restored[y, x] = residual[y, x] + sum over |dy|, |dx| <= support of model[y - dy, x - dx] * beam(dy, dx)
 * Model cells outside the image count as zero.  The taps are summed dy ascending, then dx ascending, one fused multiply-add
 * each, starting from +0.0, and the residual is added last; nothing is accumulated with atomics, so the host, _dev and
 * imager forms give the same bits, and so do two runs.  The restored image is in units per beam (the beam's peak is 1).
 * restored may be residual itself (an in-place restore); otherwise it may overlap neither residual nor model nor beam.
 * The _dev forms read the beam from 8 doubles on the device - the fit's output, or { A, B, C, -, -, -, -, ok != 0 } of
 * the caller's own: a beam whose ok is 0 or NaN, or whose A, B, C are not finite and positive definite, writes NaN to
 * every cell of restored; nothing is read back and nothing is silently replaced by a delta beam.  gridhip_restore takes
 * the 8 doubles from the host and refuses such a beam with GRIDHIP_EINVAL before anything is touched.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL handle or array (the imager form's beam
 * output may be NULL), N < 1, window < 1, cut outside (0, 1) or NaN, support < 1, a forbidden overlap.  support > 32 or
 * N above 1048560 is GRIDHIP_EUNSUPPORTED.
 * The fit is one work-group: each thread owns whole rows of the window (any window; 128 rows per pass), one thread adds the
 * rows, solves and writes the result.  The restore is an LDS-tiled direct convolution: a work-group makes 32 x 64 cells,
 * stages the model tile and its halo of `support` cells and, unless that window holds no non-zero cell - then the tile is
 * residual + 0.0, with the same bits as the full sum (a -0.0 residual becomes +0.0 either way) - the (2 support + 1)^2
 * weights, evaluated once per work-group.  gridhip_fit_beam and gridhip_restore are synchronous and stage host arrays
 * through the context's pool.  The _dev and imager forms take device pointers, enqueue one kernel each on the context's
 * stream (no memset or copy node), allocate nothing after the first call, never synchronise and read nothing back, so
 * visibilities -> deconvolve -> restore can be captured into one graph.  They need no scratch. */
int gridhip_fit_beam(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam);
int gridhip_fit_beam_dev(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam);
int gridhip_restore(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                    int64_t support, double *restored);
int gridhip_restore_dev(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                        int64_t support, double *restored);
/* gridhip_fit_beam_dev on the imager's own PSF (nothing is copied) and N */
int gridhip_imager_beam_dev(gridhip_imager *imager, int64_t window, double cut, double *beam);
/* the fit on the imager's own PSF, then gridhip_restore_dev with that beam; beam (8 doubles on the device) receives it,
 * or is NULL */
int gridhip_imager_restore_dev(gridhip_imager *imager, const double *model, const double *residual, int64_t window,
                               double cut, int64_t support, double *restored, double *beam);

/* ---- imaging weights: natural, uniform, Briggs, taper and data weights, on the device -----------------------------------
 * The reference weights one way only, doweight (src/Gridding.hs:564-583: every visibility divided by the number of
 * visibilities in its cell); everything beyond that is defined here.  For n visibilities at (u_k, v_k) in wavelengths
 * (uv_stride as everywhere; taken as given - nothing is mirrored here, a caller that wants Hermitian cells merged mirrors
 * first, as do_imaging does), N = gridhip_image_size(theta, lam), data weights s_k (wt_in: n doubles, or NULL for all
 * ones), mode, robust R and taper_sigma sigma (wavelengths; 0: no taper):
 *     FLAGGED   a visibility whose s_k is not > 0 (zero, negative, NaN): w_k is exactly +0.0 and it takes part in nothing else
 *     c_k       doweight's cell of (u_k / lam, v_k / lam); -1 outside the grid or for NaN coordinates
 *     D[c]      the sum of s_k over the unflagged visibilities with c_k = c
 *     t_k       exp(-(u_k^2 + v_k^2) / (2 sigma^2)), or 1 when sigma = 0
 *     mode 0    natural   w_k = s_k t_k
 *     mode 1    uniform   w_k = (s_k / D[c_k]) t_k
 *     mode 2    Briggs    f^2 = (5 * 10^-R)^2 / (sum_c D[c]^2 / sum_c D[c]) ;  w_k = s_k / (1 + D[c_k] f^2) t_k
 *                         (1 + D f^2 is a rounded product followed by an add: no fused multiply-add; f^2 is 0 when no
 *                         visibility lies in the grid)
 *     OUTSIDE   an unflagged visibility with c_k = -1 keeps w_k = s_k t_k in every mode, as doweight keeps 1, and is left
 *               out of D, of f^2 and of the sums below
 *     stats     8 doubles { sum w, sum w^2 / s, sum s, noise, f^2, n_used, n_flagged, n_outside }, the sums over the
 *               unflagged visibilities in the grid; noise = sqrt(sum(w^2 / s) sum(s)) / sum(w), NaN when sum w is 0: the
 *               thermal noise relative to natural weighting (>= 1, and 1 for natural weighting without a taper); f^2 is 0
 *               outside mode 2.  stats may be NULL.
 * With wt_in NULL, D is an integer count and sum D, sum D^2 are 64-bit integer sums: the weights do not depend on the
 * schedule (two calls give the same bits), and mode 1 without a taper gives the bits of doweight applied to ones,
 * 1.0 / count.  With data weights D is accumulated with fp64 atomics and the weights agree to the order of those sums
 * (1e-10 relative at up to 1000 visibilities per cell).  The six sums of stats are added in a fixed order either way.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context; NULL u, v or wt_out with n > 0;
 * n < 0; uv_stride < 1; N < 1; a mode outside 0..2; a robust that is not finite; taper_sigma < 0 or NaN; wt_out
 * overlapping u or v.  wt_out may be wt_in itself (in place).
 * gridhip_weights is synchronous and stages host arrays through the context's pool (stats: 8 doubles on the host).
 * gridhip_weights_dev takes device pointers (stats: 8 doubles on the device) and enqueues kernels only on the context's
 * stream - no memset node, no copy node: a kernel zeroes the density; pass 1 over the visibilities takes the cell and
 * accumulates the density (uint32 counts, or fp64 atomics with data weights) and leaves the 8-byte cell code; for Briggs
 * one reduction over the N^2 cells; pass 2 writes w with the sums of stats fused into it (it reads u, v again only for
 * a taper); a one-work-group kernel writes stats.  Natural weighting is pass 2 alone.  f^2 never leaves the device.  The
 * scratch (the density, 8 B per visibility of cell codes, 200 KB of partial sums) comes from the context's pool: nothing
 * is allocated after the first call of a shape, nothing is read back and nothing synchronises, so a call can be captured
 * into a graph like clean and restore. */
int gridhip_weights(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                    int64_t uv_stride, const double *wt_in, int mode, double robust, double taper_sigma, double *wt_out,
                    double *stats);
int gridhip_weights_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                        int64_t uv_stride, const double *wt_in, int mode, double robust, double taper_sigma,
                        double *wt_out, double *stats);
/* Imagers with a weighting: the creation calls above plus (mode, robust, taper_sigma, wt_in).  wt_in is n doubles on the
 * device in the un-mirrored order of vis, or NULL; the density is taken on the MIRRORED coordinates, where the imager takes
 * doweight's.  gridhip_imager_create_dev / _aw_dev are these with (1, 0, 0, NULL), bit for bit.  Everything after
 * creation - cycle, predict, psf, clean, deconvolve, beam, restore - is unchanged and sees the new weights; prediction
 * stays un-weighted.  A visibility of weight 0 (flagged) contributes EXACTLY NOTHING to the image and the PSF even when its
 * vis is NaN or Inf: its contribution is selected out, not multiplied by zero (vis_res is still vis - pred for it).
 * Memory held per visibility is unchanged: the mirror flag stays the sign bit of the stored weight, of a zero too. */
int gridhip_imager_create_weighted_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh,
                                       int64_t gw, const double *kv, double theta, int64_t lam, int64_t n,
                                       const double *u, const double *v, const double *w, int64_t uv_stride, int mode,
                                       double robust, double taper_sigma, const double *wt_in, gridhip_imager **imager);
int gridhip_imager_create_aw_weighted_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                                          int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                                          int64_t n, const double *u, const double *v, const double *w,
                                          int64_t uv_stride, const int64_t *a1, const int64_t *a2, int mode,
                                          double robust, double taper_sigma, const double *wt_in,
                                          gridhip_imager **imager);
/* the stats of the creation's weighting, copied on the stream into 8 doubles on the device */
int gridhip_imager_weight_stats_dev(gridhip_imager *imager, double *stats);

/* ---- wide-band imaging: Taylor-term major cycles and a multi-term CLEAN, on the device ---------------------------------
 * Multi-term multi-frequency synthesis (Sault & Wieringa 1994; Rau & Cornwell 2011, one scale): the sky is modelled as
 * I(nu) = sum_t I_t x^t with x = (nu - nu_0) / nu_0, T Taylor terms, 1 <= T <= 4.  The reference has nothing of the kind:
 * the semantics are defined here.
 * THE MINOR CYCLE.  All images are real N x N, laid out as gridhip_clean's, c = (N / 2, N / 2):
 *     psfs       [2T - 1][N][N], the spectral PSFs P_s
 *     residuals  [T][N][N], updated in place
 *     models     [T][N][N], accumulated into, never zeroed
 *     H[t][q] = P_{t+q}[c, c]
 *     Hinv    = the inverse of H by Gauss-Jordan WITHOUT pivoting, rows in order: the pivot row is divided by the pivot
 *               (true divisions), then m * (pivot row) is taken from every other row, m that row's entry in the pivot's
 *               column, the product rounded, then subtracted (no fused multiply-add).  A pivot that is not > 0, NaN
 *               included, makes H singular: nothing is done, reason 3, stats = { 0, NaN, -1, 0, 0, 0, 0, 3 }
 *     repeat at most niter times:
 *         for every cell:  a_t = sum_q Hinv[t][q] * R_q   (q ascending from the first product, each product rounded,
 *                                                          then added)
 *                          s   = sum_t a_t * R_t          (t ascending, likewise)
 *         k = the flat index of the largest s over border <= y, x < N - border; ties go to the lowest flat index; a NaN
 *             s is never selected.  (Hinv is positive definite when the elimination succeeds, so s is negative only by
 *             the rounding of a cell at zero: the comparison is clean's own, on the magnitude.)
 *         p = a_0[k]
 *         if |p| <= threshold: stop                                (before anything is subtracted)
 *         f_t = gain * a_t[k] (rounded once);  models[t][k] += f_t;  flux_t += f_t
 *         R_t[y', x'] = (...((R_t - f_0 * P_t) - f_1 * P_{t+1}) ... - f_{T-1} * P_{t+T-1})  at the PSF index
 *                       [y' - y + c, x' - x + c], q ascending, each product rounded before it is subtracted; the region
 *                       and the patch rule are exactly gridhip_clean's
 *     stats (8 doubles) = { iterations, a_0 at the final k*, k*, flux_0, flux_1, flux_2, flux_3, reason }, k* the peak of
 *                         the final residuals under the same rule (NaN at -1 when nothing can be selected); reason
 *                         0: niter components taken, 1: |p| <= threshold, 2: nothing selectable, 3: singular H - the
 *                         first of 3, 2, 1 that holds; unused flux slots are 0
 * (Rounding, for a restatement that wants the bits: as in gridhip_clean, models[t][k] and flux_t receive gain * a_t in one
 * fused multiply-add each; f_t itself, which scales the PSFs, is the rounded product.)
 * With T = 1 and P_0[c, c] == 1 this is Hogbom CLEAN: residual and model come out with gridhip_clean's bits wherever no
 * two cells tie in the square of their value.  No atomics anywhere, contraction is off: a call is deterministic bit for
 * bit, and the host, _dev and imager forms give the same bits.
 * Arguments: gridhip_clean's rules for N, gain, threshold, niter, border, patch and NULL pointers, its NaN rule and its
 * GRIDHIP_EUNSUPPORTED limit on N; T in 1 .. 4; no two of the 4T - 1 planes overlapping - GRIDHIP_EINVAL, refused before
 * anything is touched.
 * The shape is gridhip_clean's: tiles of 16 x 128 cells, a device table of one (score, index) entry per tile.  The first
 * launch builds the table in one pass over the T residuals, the second inverts H into the state block and takes the first
 * component; an iteration is two launches: a tile kernel over the overlapped tiles only, which reads T residuals and
 * 2T - 1 PSFs and writes T residuals - (4T - 1) * 8 B per cell, (4T - 1) / 3 of Hogbom's - and recomputes the tiles'
 * scores in the same pass, and a one-work-group kernel that reduces the table, recomputes a_t at k from the T residual
 * cells, tests the stop rule and takes the component.  gridhip_mfclean is synchronous and stages host arrays through the
 * context's pool.  The _dev forms enqueue kernels only on the context's stream (2 + 2 * niter launches; no memset or copy
 * node), allocate nothing after the first call of a shape, never synchronise and read nothing back: they can be
 * captured into a graph.  Scratch (256 B + 16 B per tile) comes from the context's pool, or for the imager form from
 * memory the imager owns.  Masks, noise-based stop levels and a multi-scale variant are not part of this form. */
int gridhip_mfclean(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                    double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats);
int gridhip_mfclean_dev(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                        double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats);
/* WIDE-BAND IMAGERS.  set_spectral gives an imager T Taylor terms: x is n doubles on the device, x_k = (nu_k - nu_0) /
 * nu_0 of visibility k in the order of vis; it is copied, and the caller may free it.  The powers are pw_0 = 1,
 * pw_t = pw_{t-1} * x.  A visibility whose x_k is not finite is treated as flagged: it grids nothing and predicts 0 in
 * every term.  The call builds and keeps the 2T - 1 spectral PSFs, DEFINED BY EXISTING CALLS:
 *     P_s = the image of cycle(NULL, vis_k = (pw_s(x_k), 0))
 * - the weighted PSF pass with x^s, divided by the imager's stored pmax - so that P_0 agrees with the imager's own PSF
 * to the tolerance of the fp64 atomics (1e-10).  It may synchronise, as creation does; calling it again replaces the
 * terms.  T outside 1 .. 4 or (n > 0) a NULL x is GRIDHIP_EINVAL.  No other entry point changes: an imager without
 * spectral terms is what it was, and one with them still cycles, cleans and restores as before.
 * Memory: an imager with spectral terms also holds 8 B (x) + 16 B (the residual visibilities of an mfs_cycle) per
 * visibility, 2T - 1 images of N^2 doubles and, after its first mfclean, 256 B + 16 B per 16 x 128 cells. */
int gridhip_imager_set_spectral_dev(gridhip_imager *imager, int64_t T, const double *x);
/* the 2T - 1 spectral PSFs, [2T - 1][N][N] doubles on the device, copied on the stream */
int gridhip_imager_spectral_psfs_dev(gridhip_imager *imager, double *psfs);
/* one wide-band major-cycle step, DEFINED BY THE CALLS IT REPLACES (models [T][N][N] or NULL, images [T][N][N]):
 *     r         = vis - sum_q pw_q(x) * predict(models[q])     (q ascending; models NULL: r = vis)
 *     images[t] = cycle(NULL, pw_t(x) * r).image               vis_res, when given, = r (it may be vis itself)
 * One forward transform and one gather per model term, accumulated into the residual-visibility block; then per term one
 * pass over that block (times pw_t, conjugate where mirrored, times the weight), the scatter and the tail.
 * Asynchronous, allocation-free after the first call, kernels only, capturable, like cycle. */
int gridhip_imager_mfs_cycle_dev(gridhip_imager *imager, const double *models, const double *vis, double *images,
                                 double *vis_res);
/* gridhip_mfclean_dev with the imager's spectral PSFs (nothing is copied), its T and N */
int gridhip_imager_mfclean_dev(gridhip_imager *imager, double *residuals, double *models, double gain, double threshold,
                               int64_t niter, int64_t border, int64_t patch, double *stats);
/* visibilities -> T model images in one call, DEFINED BY THE CALLS IT REPLACES:
 *     repeat nmajor times: images = mfs_cycle(models, vis); mfclean(images, models) with stats + 8 * i (when stats != NULL)
 *     images = mfs_cycle(models, vis)
 * models is the caller's and must be initialised; stats is nmajor x 8 doubles on the device, or NULL.
 * spectral_psfs, mfs_cycle, mfclean and mfdeconvolve on an imager without spectral terms are GRIDHIP_EINVAL. */
int gridhip_imager_mfdeconvolve_dev(gridhip_imager *imager, const double *vis, double *models, double *images,
                                    int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                    int64_t patch, double *stats);

/* ---- gain calibration: per-antenna gains by StEFCal, their application, and a selfcal step, on the device ----------------
 * The reference has no calibration: the semantics are defined here.  Scalar, single-polarisation, direction-independent
 * antenna gains (StEFCal: Salvini & Wijnholds 2014; 2x2 Jones matrices: "polarisation" below) with solution intervals.
 * Inputs: n visibilities V_k (vis) and model
 * visibilities M_k (model_vis), complex as interleaved doubles; the antenna pairs p_k = a1[k], q_k = a2[k], each in
 * [0, A); the solution interval t_k = slot[k] in [0, T), or slot == NULL with T == 1; data weights s_k (wt: n doubles, or
 * NULL for all ones).  The measurement equation is V_k ~ g[t,p] M_k conj(g[t,q]); gains is [T][A] complex.
 *     FLAGGED   a visibility whose s_k is not > 0 (zero, negative, NaN) - gridhip_weights' rule, looked at first: it
 *               contributes exactly nothing even when V_k or M_k is NaN or Inf (selected out, not multiplied by zero)
 *     DROPPED   an unflagged visibility whose p, q or t is out of range: it contributes nothing and is counted
 *     AUTO      an unflagged one in range with p == q: it contributes nothing and is counted with the dropped
 *     X_k = (s_k V_k) conj(M_k),  Y_k = s_k |M_k|^2      once per solve, every product rounded (no fused multiply-add):
 *               (a + bi) conj(c + di) = (a c + b d) + (b c - a d) i with a + bi = (s re V, s im V);  |M|^2 = c c + d d
 *     start     g = 1 everywhere, or the caller's gains when warm != 0
 *     iteration i = 0, 1, ... with the current g, for every (t, a):
 *               num[t,a] = sum_{t_k = t, p_k = a} X_k g[t,q_k]      + sum_{t_k = t, q_k = a} conj(X_k) g[t,p_k]
 *               den[t,a] = sum_{t_k = t, p_k = a} Y_k |g[t,q_k]|^2  + sum_{t_k = t, q_k = a} Y_k |g[t,p_k]|^2
 *               g'[t,a]  = num / den where den > 0; else g'[t,a] = g[t,a], the very bits, and none of the next two
 *                          rules touches it (UNSOLVED in this iteration)
 *               mode 1 (phase only): g' <- g' / |g'| where |g'| > 0, else g
 *               on odd i: g' <- (g' + g) / 2
 *               rel = sqrt(sum |g' - g|^2 / sum |g'|^2) over all (t, a);  then g <- g'
 *               stop when tol > 0 and rel <= tol: rel is tested after the update, and tol = 0 never stops early
 *     after the loop (t, a) is UNSOLVED when its den was never > 0: its gain is exactly 1 + 0i (or the warm value), and
 *               it is counted.  If refant >= 0 every solved gain of an interval is multiplied by conj(g[t,refant]) /
 *               |g[t,refant]|, and g[t,refant] itself becomes (|g[t,refant]|, 0): real and non-negative.  The rotation
 *               leaves an unsolved gain the very bits it started from, and an interval whose reference antenna is
 *               unsolved (or zero, or not finite) is left unrotated.  refant < 0: no rotation.
 *     stats     8 doubles { iterations performed, the last rel (NaN when there was none), chi^2 = sum s_k |V_k - g_p M_k
 *               conj(g_q)|^2 over the used k with the final gains, chi^2 at g = 1, n_used, n_flagged, n_dropped (autos
 *               included), the number of unsolved (t, a) }.  stats may be NULL.
 * APPLY takes gains [T][A], vis_in, a1, a2, slot and optionally wt_in (NULL: ones) and wt_out (NULL: not written):
 *     inverse 1 (correct data)     vis_out = vis_in / (g_p conj(g_q)),  wt_out = wt_in |g_p|^2 |g_q|^2.  A visibility whose
 *               p, q or t is out of range, or that touches a gain that is zero or not finite, gets vis_out = vis_in and
 *               wt_out = +0.0: gridhip_weights' flag, so that a corrected stream leaves out the baselines to an
 *               antenna without a gain.  "Zero or not finite" is judged on |g|^2 as fp64 computes it, so a gain whose
 *               square underflows to 0 or overflows (|g| below about 1e-154 or above about 1e154) counts as such.
 *     inverse 0 (corrupt a model)  vis_out = g_p vis_in conj(g_q), weights copied; out of range: vis_out = vis_in.
 *     Autocorrelations and flagged visibilities are applied like any other.  In place (vis_out == vis_in, wt_out ==
 *     wt_in) is allowed; any other overlap of an output with an input or with the other output is refused.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context; n < 0; A < 2; T < 1; slot ==
 * NULL with T != 1; a NULL a1, a2, vis, model_vis (gaincal), vis_in, vis_out (apply) with n > 0; a NULL gains; niter < 0;
 * tol < 0 or NaN; a mode or an inverse outside 0..1; refant >= A; gains overlapping any input (gaincal) or any output
 * (apply).  n = 0 is valid: the gains are all 1 (or the warm values) and everything is unsolved.  A * T above 2^21
 * (2097152; A = 512 with T = 4096) is GRIDHIP_EUNSUPPORTED: a solve keeps 28 B of scratch per (t, a) and its two
 * one-work-group kernels pass over all of them in every iteration.
 * gridhip_gaincal and gridhip_apply_gains are synchronous and stage host arrays through the context's pool.  The _dev
 * and imager forms take device pointers and enqueue kernels only on the context's stream - no memset node, no copy node;
 * they allocate nothing after the first call of a shape (the scratch - 32 B per visibility, 28 B per (t, a) - comes from
 * the context's pool), never synchronise and read nothing back.  The stop condition lives on the device as in
 * gridhip_clean: niter iterations are enqueued unconditionally and a launch that finds the state stopped returns at its
 * first instruction, so a solve or a whole selfcal can be captured into a graph like clean and restore.
 * A solve is: one pass that reads V, M, s, a1, a2, slot and leaves X (16 B), Y (8 B) and a packed 8-byte key (t, p, q,
 * used) per visibility; per iteration a kernel that streams those 32 B - a work-group takes a contiguous range of whole
 * chunks of 4096 visibilities, keeps the gains and the (num, den) sums of one interval in LDS (A <= 512; more antennas
 * add to global memory directly) and flushes to a global [T][A][3] table when the interval changes, so a time-major
 * stream is the fast case and an unordered slot is merely slower - and a one-work-group kernel that forms g', rel and the
 * stop test and zeroes the table; then the rotation, and one more pass for chi^2.
 * DETERMINISM.  The sums over the visibilities meet in fp64 atomics: gains are reproducible to the order of those sums
 * (1e-10 of the largest |g| at a few thousand visibilities per antenna), as gridhip_weights with data weights - NOT bit
 * for bit.  Given the gains, rel, chi^2 and the counts are added in a fixed order. */
int gridhip_gaincal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                    int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int gridhip_gaincal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                        int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int gridhip_apply_gains(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                        double *vis_out, double *wt_out);
int gridhip_apply_gains_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                            const int64_t *slot, const double *gains, int inverse, const double *vis_in,
                            const double *wt_in, double *vis_out, double *wt_out);
/* One self-calibration step of an imager of any kind, DEFINED BY THE CALLS IT REPLACES:
 *     pred = gridhip_imager_predict_dev(imager, model, NULL)
 *     gridhip_gaincal_dev(vis against pred)                         -> gains, stats
 *     gridhip_apply_gains_dev(inverse = 1, vis, wt)                 -> vis_cal, wt_cal (wt_cal may be NULL)
 * n is the imager's; a1, a2 (for the aw kind too: the imager does not keep them in the order of vis), slot, wt, vis,
 * gains [T][A], vis_cal and wt_cal are on the device.  The solver reads the imager's own prediction where the gather left
 * it - nothing is copied - and the solve's last pass writes the corrected stream.  vis_cal may be vis and wt_cal may be
 * wt.  vis_cal can go straight into cycle or deconvolve; wt_cal is what a re-weighted imager would be created with.  A
 * NULL imager or model is GRIDHIP_EINVAL; the other rules are those of the two calls. */
int gridhip_imager_selfcal_dev(gridhip_imager *imager, const double *model, const double *vis, int64_t A, int64_t T,
                               const int64_t *a1, const int64_t *a2, const int64_t *slot, const double *wt, int mode,
                               int64_t refant, int warm, int64_t niter, double tol, double *gains, double *vis_cal,
                               double *wt_cal, double *stats);

/* ---- direction-dependent calibration: D gain sets per antenna at once, the subtraction of directions, a peel step ----------
 * The reference has no calibration: the semantics are defined here, on top of "gain calibration" above.  The sky is split
 * into D directions, 1 <= D <= 8, each with its own model visibilities and its own gains: model_vis is [D][n] complex,
 * contiguous (row d: the model of direction d), gains is [D][T][A] complex, and the measurement equation is
 *     V_k ~ sum_d g[d,t_k,p_k] M[d,k] conj(g[d,t_k,q_k])
 * n, A, T, a1, a2, slot, vis, wt, mode, refant, warm, niter, tol and stats are gridhip_gaincal's.  The classes FLAGGED,
 * DROPPED and AUTO are exactly those of gridhip_gaincal (a flagged visibility contributes exactly nothing even when V_k
 * or any M[d,k] is NaN or Inf), and so are the start (g = 1 everywhere, or the caller's gains when warm != 0) and the stop
 * test on the device.  The solver is the multi-direction StEFCal (the "direction solve" of Smirnov & Tasse 2015, as in
 * DP3): iteration i = 0, 1, ... with the current g, for every (t, a), over the used k with t_k = t:
 *     for each k with p_k = a:  z_d = M[d,k] conj(g[d,t,q_k]),        y = V_k
 *     for each k with q_k = a:  z_d = conj(M[d,k]) conj(g[d,t,p_k]),  y = conj(V_k)
 *     H[d,e] = sum s_k conj(z_d) z_e   Hermitian; the upper triangle is kept: D real diagonals, D (D - 1) / 2 complex entries
 *     b[d]   = sum s_k conj(z_d) y
 *     g'[.,t,a] solves H g' = b by LDL^H without pivoting, in direction order: H = L diag(d_j) L^H, L unit lower
 *               triangular, d_j = H[j,j] - sum_{k<j} |L[j,k]|^2 d_k.
 *     SOLVED    (t, a) is solved in this iteration iff every pivot d_j > 1e-12 * H[j,j], the product as fp64 computes it
 *               (a NaN fails the test).  Otherwise ALL D gains of (t, a) keep their bits and none of the next rules
 *               touches them (UNSOLVED in this iteration, as in gridhip_gaincal): a direction without a model on the
 *               baselines of an antenna, two equal directions, or fewer independent visibilities than directions.
 *     mode 1 (phase only): each g'[d] <- g'[d] / |g'[d]| where |g'[d]| > 0, else g[d] - every direction separately
 *     on odd i: g' <- (g' + g) / 2
 *     rel = sqrt(sum |g' - g|^2 / sum |g'|^2) over all (d, t, a);  then g <- g';  stop when tol > 0 and rel <= tol
 *     after the loop (t, a) is UNSOLVED when it was solved in no iteration: its D gains are exactly 1 + 0i (or the warm
 *               values), and it is counted once.  If refant >= 0 the rotation of gridhip_gaincal is done per direction
 *               and per interval: every gain g[d,t,.] of a solved (t, a) is multiplied by conj(g[d,t,refant]) /
 *               |g[d,t,refant]| and g[d,t,refant] becomes real and non-negative; where (t, refant) is unsolved, or
 *               g[d,t,refant] is zero or not finite, that direction of that interval is left unrotated.
 *     stats     8 doubles in gridhip_gaincal's layout; chi^2 = sum s_k |V_k - sum_d g[d,t,p] M[d,k] conj(g[d,t,q])|^2 over
 *               the used k, at the final gains and at g = 1; "unsolved" counts the (t, a) that were never solved.
 * With D = 1 the iteration is gridhip_gaincal's formula, g' = sum X g_q / sum Y |g_q|^2, up to the order of the products.
 * Products: s_k V_k is formed once per solve; per iteration z_d, s_k z_d, conj(z_d) (s_k z_e) and conj(z_d) (s_k y), every
 * product rounded (no fused multiply-add).
 * All arguments are checked before anything is touched.  GRIDHIP_EINVAL: every refusal of gridhip_gaincal (with gains and
 * model_vis at their larger sizes in the overlap test), and D outside 1..8.  D * A * T above 2^21 is
 * GRIDHIP_EUNSUPPORTED.  n = 0 is valid.
 * gridhip_ddcal is synchronous and stages host arrays through the context's pool.  gridhip_ddcal_dev takes device
 * pointers and enqueues kernels only on the context's stream - no memset node, no copy node; it allocates nothing after
 * the first call of a shape (the scratch - 32 B per visibility, (D^2 + 2 D) * 8 + 4 B per (t, a) - comes from the
 * context's pool), never synchronises and reads nothing back: niter iterations are enqueued unconditionally and a launch
 * that finds the state stopped returns at its first instruction, so a solve can be captured into a graph.
 * A solve is: one pass that leaves s V (16 B), s (8 B) and the packed 8-byte key per visibility; per iteration a kernel,
 * one instantiation per D, that streams those 32 B and the D model values (48 B per visibility at D = 1, where gaincal
 * streams 32 B) - a work-group takes a contiguous range of whole chunks of 4096 visibilities, keeps the gains (2 D doubles)
 * and the sums (D^2 + 2 D doubles) of one interval in LDS, (D^2 + 4 D) * 8 bytes per antenna, adds with LDS fp64 atomics
 * and flushes to a global [T][A][D^2 + 2 D] table when the interval changes - and a one-work-group kernel with one thread
 * per (t, a) that does the LDL^H, the mode, the averaging, rel and the stop test and zeroes the table; then the rotation,
 * and one more pass for chi^2.
 * LDS BUDGET.  The LDS path serves A <= gridhip_ddcal_lds_antennas(D) = floor(131072 / ((D^2 + 4 D) * 8)): 3276, 1365,
 * 780, 512, 364, 273, 212, 170 for D = 1 .. 8; more antennas add to the global table directly.  The budget is 128 KiB of
 * the 160 KiB a gfx950 CU has: a table above 80 KiB leaves room for one work-group per CU anyway, so the budget is set by
 * what that one work-group still needs beside it (nothing but a word), rounded down to the power of two that admits
 * A = 512 at D = 4; the kernel then runs as ONE work-group of 1024 threads per CU, two of 512 from 40 KiB, four of 256
 * below, so that a CU holds 1024 threads whatever the table takes.  gridhip_ddcal_lds_antennas is a pure host function;
 * it returns 0 for D outside 1..8.
 * DETERMINISM.  The sums over the visibilities meet in fp64 atomics: gains are reproducible to the order of those sums
 * (1e-10 of the largest |g| at a few thousand visibilities per antenna, for an H whose pivots are far from the threshold)
 * - NOT bit for bit.  Given the gains, rel, chi^2 and the counts are added in a fixed order. */
int gridhip_ddcal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                  const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                  int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int gridhip_ddcal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                      int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int64_t gridhip_ddcal_lds_antennas(int64_t D);
/* SUBTRACT takes gains [D][T][A], model_vis [D][n], a1, a2, slot, a set of directions dirs (bit d: direction d; a 64-bit
 * mask passed as int64_t) and vis_in:
 *     vis_out = vis_in - sum_{d in dirs, ascending} g[d,t,p] M[d,k] conj(g[d,t,q])
 * the terms subtracted one after the other, each (g_p M) conj(g_q) with every product rounded (no fused multiply-add).
 * vis_in == NULL means zeros with the sign flipped: vis_out = + the same sum, started from +0 - the corrupted model itself,
 * the counterpart of gridhip_apply_gains(inverse = 0).  A visibility whose p, q or t is out of range gets vis_out = vis_in
 * (or 0); autocorrelations and flagged visibilities are treated like any other.  In place (vis_out == vis_in) is allowed;
 * any other overlap of vis_out with an input is refused.  GRIDHIP_EINVAL: a NULL context; n < 0; A < 2; T < 1; D outside
 * 1..8; slot == NULL with T != 1; a NULL a1, a2, model_vis or vis_out with n > 0; a NULL gains; a bit of dirs at or above
 * D (a negative dirs has bit 63).  D * A * T above 2^21 is GRIDHIP_EUNSUPPORTED.  dirs == 0 copies.  Correction TOWARD a
 * direction stays gridhip_apply_gains on the contiguous slice gains + d * T * A * 2: there is no other apply call. */
int gridhip_dd_subtract(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs,
                        const double *vis_in, double *vis_out);
int gridhip_dd_subtract_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1,
                            const int64_t *a2, const int64_t *slot, const double *gains, const double *model_vis,
                            int64_t dirs, const double *vis_in, double *vis_out);
/* One peel step of an imager of any kind, DEFINED BY THE CALLS IT REPLACES:
 *     gridhip_imager_predict_dev(imager, model, NULL, model_vis)           -> row 0 of model_vis; rows 1 .. D - 1 are the
 *                                                                           caller's (gridhip_dft_predict of bright components)
 *     gridhip_ddcal_dev(vis against the D rows)                            -> gains [D][T][A], stats
 *     gridhip_dd_subtract_dev(dirs = directions 1 .. D - 1, vis)           -> vis_cal
 *     gridhip_apply_gains_dev(gains[0], inverse = 1, vis_cal, wt)          -> vis_cal, wt_cal (wt_cal may be NULL)
 * n is the imager's; everything is on the device, nothing is copied, the call is asynchronous and can be captured after
 * a first call.  vis_cal may be vis and wt_cal may be wt; row 0 of model_vis is written and may overlap nothing else.
 * vis_cal goes straight into cycle or deconvolve.  With D = 1 this is gridhip_imager_selfcal_dev.  A NULL imager or model
 * is GRIDHIP_EINVAL; the other rules are those of the calls. */
int gridhip_imager_peel_dev(gridhip_imager *imager, const double *model, const double *vis, int64_t A, int64_t T, int64_t D,
                            const int64_t *a1, const int64_t *a2, const int64_t *slot, const double *wt, int mode,
                            int64_t refant, int warm, int64_t niter, double tol, double *model_vis, double *gains,
                            double *vis_cal, double *wt_cal, double *stats);

/* ---- polarisation: 2x2 Jones matrices per antenna by the matrix StEFCal, their application, correlations <-> Stokes --------
 * The reference has no calibration: the semantics are defined here, on top of "gain calibration" above.  A sample is four
 * correlations: vis and model_vis are [n][2][2] complex, row-major - XX, XY, YX, YY (or RR, RL, LR, LL) as interleaved
 * doubles, 64 B per sample; gains is [T][A][2][2] complex, a Jones matrix G[t,a] per (interval, antenna).  The measurement
 * equation is V_k ~ G[t,p] M_k G[t,q]^H.  n, A, T, a1, a2, slot, wt (ONE weight per sample, shared by its four
 * correlations), refant, warm, niter, tol and stats are gridhip_gaincal's, and so are the classes FLAGGED, DROPPED and AUTO:
 * a flagged sample contributes exactly nothing even when any of its eight numbers, or of the model's, is NaN or Inf
 * (selected out, not multiplied by zero).  There are no per-correlation flags: a sample with one bad correlation is flagged
 * by its weight.
 * PRODUCTS.  Every 2x2 product is C[i][j] = X[i][0] Y[0][j] + X[i][1] Y[1][j]: two complex products, each (a c - b d) +
 * (a d + b c) i with every product and every sum rounded (no fused multiply-add), then added.  X^H is exact (transpose,
 * the imaginary signs flipped).  |X|_F^2 = ((|x00|^2 + |x01|^2) + |x10|^2) + |x11|^2, |x|^2 = re re + im im.
 *     start     G = I everywhere, or the caller's gains when warm != 0; in modes 1 and 2 the off-diagonal entries of the
 *               start are replaced by +0.0
 *     iteration i = 0, 1, ... with the current G, for every used k with s = s_k, p, q, t:
 *               toward p:  Z = M_k G[t,q]^H;    sZ = s Z entry by entry;  num[t,p] += V_k (sZ)^H;    den[t,p] += Z (sZ)^H
 *               toward q:  Z = M_k^H G[t,p]^H;  sZ = s Z;                 num[t,q] += V_k^H (sZ)^H;  den[t,q] += Z (sZ)^H
 *               den is Hermitian: d00 and d11 (the real parts of its diagonal) and d01 (complex) are kept, 4 doubles
 *               beside the 8 of num.
 *               mode 0 (full Jones): (t, a) is SOLVABLE in this iteration iff d00 > 0, d11 > 0 and e > 1e-12 * d11 with
 *               e = d11 - |d01|^2 / d00, the second pivot of the LDL^H of den without pivoting (a NaN fails).  Then
 *               G' = num den^-1 by that LDL^H: with c = d01 / d00, for each row (n0, n1) of num the row of G' is
 *               x1 = (n1 - n0 c) / e,  x0 = n0 / d00 - x1 conj(c).  Else G' = G, the very bits, and none of the rules
 *               below touches it (UNSOLVED in this iteration).
 *               mode 1 (diagonal): solvable iff d00 > 0 and d11 > 0.  G'00 = num00 / d00, G'11 = num11 / d11, the
 *               off-diagonals are +0.0: the same sums with only their diagonals used - the per-feed StEFCal over all
 *               four correlations.
 *               mode 2 (diagonal, phase only): mode 1, then each diagonal entry is divided by its modulus where that is
 *               > 0, else it is G's entry (gridhip_gaincal's rule).
 *               on odd i: G' <- (G' + G) / 2 entry by entry
 *               rel = sqrt(sum |G' - G|_F^2 / sum |G'|_F^2) over all (t, a);  then G <- G';  stop when tol > 0 and
 *               rel <= tol
 *     after the loop (t, a) is UNSOLVED when it was never solvable: its gain is exactly the start's, and it is counted.
 *               If refant >= 0, every entry of every solved G[t,a] of an interval is multiplied by the one scalar
 *               conj(r) / |r| with r = G[t,refant][0][0] (the off-diagonals of modes 1 and 2 stay +0.0), and
 *               G[t,refant][0][0] itself becomes (|r|, 0).  An interval whose reference antenna is unsolved, or whose r
 *               is zero or not finite, is left unrotated.  Only a common phase is taken out: it is the only gauge
 *               freedom that holds for an arbitrary polarised model (G -> G U needs U M_k U^H = M_k for every k).
 *     stats     8 doubles in gridhip_gaincal's layout; chi^2 = sum s_k |V_k - (G_p M_k) G_q^H|_F^2 over the used k, at the
 *               final gains and at G = I (|V_k - M_k|_F^2); "unsolved" counts the (t, a) that were never solvable.
 * With G = g I and M_k = m_k I the iteration is gridhip_gaincal's on the scalar stream, up to the order of the products;
 * mode 2 is then its phase-only mode.
 * All arguments are checked before anything is touched.  GRIDHIP_EINVAL: every refusal of gridhip_gaincal, with mode in
 * 0..2 and gains, vis and model_vis at their sizes here in the overlap test (gains overlapping an input is refused).
 * A * T above 2^21 is GRIDHIP_EUNSUPPORTED.  n = 0 is valid.
 * gridhip_jonescal is synchronous and stages host arrays through the context's pool.  gridhip_jonescal_dev takes device
 * pointers and enqueues kernels only on the context's stream - no memset node, no copy node; it allocates nothing after
 * the first call of a shape (the scratch - 16 B per visibility, 100 B per (t, a) - comes from the context's pool), never
 * synchronises and reads nothing back: niter iterations are enqueued unconditionally and a launch that finds the state
 * stopped returns at its first instruction, so a solve can be captured into a graph as one linear chain.
 * A solve is: one pass that classifies the samples and leaves the packed 8-byte key and the weight per visibility; per
 * iteration a kernel that streams those 16 B and the caller's V and M (144 B per visibility, where gaincal streams 32 B:
 * no product of V and M can be formed once per solve, the gain stands between them) - a work-group takes a contiguous
 * range of whole chunks of 4096 visibilities, keeps the gains (8 doubles) and the sums (12 doubles) of one interval in
 * LDS, 160 bytes per antenna, adds with LDS fp64 atomics (24 per visibility) and flushes to a global [T][A][12] table when
 * the interval changes - and a one-work-group kernel that forms G', rel and the stop test and zeroes the table; then the
 * rotation, and one more pass for chi^2.
 * LDS BUDGET.  The LDS path serves A <= gridhip_jonescal_lds_antennas() = 512, 80 KiB of the 160 KiB a gfx950 CU has: the
 * limit of gridhip_gaincal, so that an array either solver keeps in LDS the other does too.  A CU holds 1024 threads of the
 * kernel whatever the table takes: as many work-groups as tables (and a word each) fit, each the larger for it - four of
 * 256 threads up to A = 255, two of 512 up to A = 511, one of 1024 at A = 512.  More antennas add to the global table
 * directly.  gridhip_jonescal_lds_antennas is a pure host function.
 * DETERMINISM.  As gridhip_gaincal: the sums over the visibilities meet in fp64 atomics, so gains are reproducible to the
 * order of those sums (1e-10 of the largest |G| entry) - NOT bit for bit.  Given the gains, rel, chi^2 and the counts are
 * added in a fixed order. */
int gridhip_jonescal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                     const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                     int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int gridhip_jonescal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                         const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                         int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats);
int64_t gridhip_jonescal_lds_antennas(void);
/* APPLY takes gains [T][A][2][2], vis_in [n][2][2], a1, a2, slot and optionally wt_in (NULL: ones) and wt_out (NULL: not
 * written); the arguments are gridhip_apply_gains' with the layouts above.
 *     inverse 1 (correct data)     vis_out = (G_p^-1 vis_in) (G_q^-1)^H with G^-1 = adj(G) / det G: det = g00 g11 - g01 g10,
 *               every entry of adj(G) = [[g11, -g01], [-g10, g00]] times conj(det), divided by |det|^2.
 *               wt_out = (wt_in sqrt(|det G_p|^2)) sqrt(|det G_q|^2), which is gridhip_apply_gains' wt |g_p|^2 |g_q|^2 for
 *               G = g I; for a general Jones matrix it is the scalar approximation of a noise covariance that is no
 *               longer diagonal.  A sample whose p, q or t is out of range, or that touches a gain whose |det|^2, as fp64
 *               computes it, is zero or not finite (singular, underflowing or overflowing), gets vis_out = vis_in and
 *               wt_out = +0.0.
 *     inverse 0 (corrupt a model)  vis_out = (G_p vis_in) G_q^H, weights copied; out of range: vis_out = vis_in.
 *     Autocorrelations and flagged samples are applied like any other.  In place (vis_out == vis_in, wt_out == wt_in) is
 *     allowed; any other overlap of an output with an input or with the other output is refused.  The refusals are
 *     gridhip_apply_gains'. */
int gridhip_apply_jones(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                        double *vis_out, double *wt_out);
int gridhip_apply_jones_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                            const int64_t *slot, const double *gains, int inverse, const double *vis_in,
                            const double *wt_in, double *vis_out, double *wt_out);
/* STOKES is the bridge to everything that holds one scalar stream.  vis is [n][2][2] complex, stokes is [4][n] complex -
 * the rows I, Q, U, V, each a contiguous stream that goes into an imager, gridhip_weights, gridhip_flag_residuals,
 * gridhip_average or gridhip_gaincal as it is.  basis 0 is linear (XX, XY, YX, YY), 1 circular (RR, RL, LR, LL); which is
 * a bit mask 1..15 over I (1), Q (2), U (4), V (8).  inverse 0 reads vis and writes the selected rows of stokes; the others
 * are not touched.  With a, b, c, d the correlations 00, 01, 10, 11, real and imaginary parts separately, each sum rounded
 * once and the halving exact:
 *     linear    I = (a + d) / 2,  Q = (a - d) / 2,  U = (b + c) / 2,  V = (b - c) / (2i)
 *     circular  I = (a + d) / 2,  V = (a - d) / 2,  Q = (b + c) / 2,  U = (b - c) / (2i)
 *     (x + yi) / (2i) = (y / 2) - (x / 2) i:  re = (im b - im c) / 2,  im = (re c - re b) / 2
 * inverse 1 reads all four rows (which must be 15) and writes vis:
 *     linear    a = I + Q,  d = I - Q,  b = U + iV,  c = U - iV
 *     circular  a = I + V,  d = I - V,  b = Q + iU,  c = Q - iU
 *     x + i y = (re x - im y) + (im x + re y) i,  x - i y = (re x + im y) + (im x - re y) i
 * This is how four per-Stokes predictions become the model_vis of gridhip_jonescal.  No weights are read or written: the
 * one weight per sample serves all four streams.  GRIDHIP_EINVAL: a NULL context; n < 0; which outside 1..15; basis or
 * inverse outside 0..1; inverse with which != 15; a NULL vis or stokes with n > 0; vis overlapping the [4][n] block. */
int gridhip_stokes(gridhip_ctx *ctx, int64_t n, int basis, int which, int inverse, double *vis, double *stokes);
int gridhip_stokes_dev(gridhip_ctx *ctx, int64_t n, int basis, int which, int inverse, double *vis, double *stokes);

/* ---- residual flagging: robust per-group clipping of visibility residuals, on the device -----------------------------------
 * The reference has no flagging: the semantics are defined here.  Every other step treats a visibility whose weight is not
 * > 0 as absent; this is the step that decides that a sample is bad and produces such weights.  Inputs: n visibilities
 * V_k (vis) and model visibilities M_k (model_vis, or NULL: zero), complex as interleaved doubles; data weights s_k (wt_in:
 * n doubles, or NULL for all ones); the group g_k = group[k] (n int64: a baseline, a solution interval, ...), or group ==
 * NULL with G == 1; G groups; nsigma, amax, min_count, niter.
 * CLASSES.  Each visibility falls into the FIRST class that applies; its code goes to flags_out (n bytes, may be NULL):
 *     1       FLAGGED ON INPUT  s_k is not > 0 (zero, negative, NaN) - gridhip_weights' rule, looked at first: it takes
 *             part in nothing, whatever V_k, M_k or g_k hold
 *     2       LEFT ALONE        g_k < 0 or g_k >= G: not tested, not counted in any group, its weight passes through
 *             unchanged - how a caller exempts samples
 *     3       NOT FINITE        a_k (below) is NaN or Inf.  As in gridhip_apply_gains this is judged on the value fp64
 *             computes: a component of the residual above about 1e154 squares to Inf and counts
 *     4       ABOVE AMAX        amax > 0 and a_k > amax
 *     16 + r  CLIPPED in round r (below)
 *     0       KEPT
 * AMPLITUDE.  r_k = V_k - M_k, each component one rounded subtraction;  a_k = sqrt(re * re + im * im): both products
 *     rounded, the sum rounded, no fused multiply-add, a correctly rounded square root - numpy's np.sqrt(re * re + im * im)
 *     to the bit (NOT np.abs, which is hypot).  a_k >= +0.0, so the unsigned bit pattern of a_k is its order-preserving
 *     key; the same holds for d_k = |a_k - med|.
 * ROUNDS r = 0 .. niter - 1 over the PARTICIPANTS, the visibilities still of class 0.  For every group g:
 *     n_g     the number of participants of the group
 *     med_g   the LOWER median of their a_k, the element of rank (n_g - 1) / 2: an element, never an average
 *     MAD_g   the lower median of d_k = |a_k - med_g|, each rounded once
 *     sigma_g = 1.4826 * MAD_g;   T_g = med_g + nsigma * sigma_g, the product rounded, then the sum
 *     T_g = +Inf when n_g < min_count or sigma_g == 0: a group of ties, or one too small, is not clipped
 *     a participant with a_k > T_g gets the code 16 + r and is no participant any more
 *     A round that clips nothing stops the loop.  niter = 0 is valid: the classes 1 to 4 only, no statistics.
 * OUTPUTS.  wt_out (n doubles; may be wt_in itself) holds s_k (1 without data weights) for the classes 0 and 2 and exactly
 *     +0.0 otherwise; vis is never written.  group_stats ([G][4] doubles, may be NULL) holds { n_g, med_g, MAD_g, T_g } of
 *     the last round that ran, as that round saw them; an empty group gives { 0, NaN, NaN, +Inf }, and with niter = 0
 *     every group has that form with its count.  stats (8 doubles, may be NULL): { rounds run (the one that clipped
 *     nothing included), participants at the start of round 0, clipped in all rounds, not finite, above amax, left alone,
 *     flagged on input, kept }.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context; n < 0; G < 1; group == NULL with
 * G != 1; a NULL vis or wt_out with n > 0; nsigma not finite or <= 0; amax NaN or < 0; min_count < 1; niter < 0 or > 16;
 * any output overlapping an input or another output, other than wt_out == wt_in.  G above 2^18 (262144; A = 512 antennas
 * give 130816 baselines) is GRIDHIP_EUNSUPPORTED - the bin table is 1 KB per group - and so is n above 2^32 - 1 (the bins
 * and ranks are 32-bit counts).  n = 0 is valid.
 * gridhip_flag_residuals is synchronous and stages host arrays through the context's pool.  The _dev and imager forms take
 * device pointers and enqueue kernels only on the context's stream - no memset node, no copy node (the tables are zeroed
 * by kernels); they allocate nothing after the first call of a shape (the scratch - 12 B per visibility, 1 KB of bins and
 * 40 B of state per group - comes from the context's pool, or is the imager's own), never synchronise and read nothing
 * back.  The stop test lives on the device as in gridhip_clean and gridhip_gaincal: all niter rounds are enqueued, a round
 * counts what it clips, and every launch of the next round reads that count first and returns at once when it is zero -
 * so a call can be captured into a graph.  The launch count, 3 + 33 niter (5 for niter = 0), does not depend on the data.
 * A call is: one pass that reads V, M, s and g (40 B) and leaves the 8-byte key of a_k and a 4-byte group code per
 * visibility; per round a segmented most-significant-digit radix select with 8-bit digits over those 12 B - 8 passes for
 * the medians of all groups at once, then 8 over d_k for the MADs, each followed by a kernel that takes, one wave per
 * group, the digit that holds the group's rank - and a pass that clips; then a pass that writes wt_out.  The histogram
 * has two paths, chosen by G alone: for G <= 64 a work-group keeps G x 256 32-bit bins in LDS (1 KB per group) and adds
 * its non-zero bins to the global table; above 64 the lanes add to the global [G][256] table directly.
 * DETERMINISM.  Every output is an order statistic, a count, or one rounded expression of those: integer atomics only, no
 * floating-point atomic, no sum of doubles.  The result is the same bits for the host, _dev and imager forms, for two
 * runs, on either histogram path, and for a numpy restatement that sorts. */
int gridhip_flag_residuals(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis,
                           const double *model_vis, const double *wt_in, double nsigma, double amax, int64_t min_count,
                           int64_t niter, double *wt_out, uint8_t *flags_out, double *group_stats, double *stats);
int gridhip_flag_residuals_dev(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis,
                               const double *model_vis, const double *wt_in, double nsigma, double amax,
                               int64_t min_count, int64_t niter, double *wt_out, uint8_t *flags_out, double *group_stats,
                               double *stats);
/* Flagging against an imager's own prediction, for an imager of any kind, DEFINED BY THE CALLS IT REPLACES:
 *     pred = gridhip_imager_predict_dev(imager, model, NULL)
 *     gridhip_flag_residuals_dev(vis against pred)                  -> wt_out, flags_out, group_stats, stats
 * n is the imager's; vis, group, wt_in and the outputs are on the device.  The front pass reads the imager's own
 * prediction where the gather left it, as selfcal does - nothing is copied - and the scratch is the imager's.  wt_out is
 * what a re-weighted imager is created with, or what gridhip_imager_selfcal_dev takes as wt.  A NULL imager or model is
 * GRIDHIP_EINVAL; the other rules are those of gridhip_flag_residuals_dev. */
int gridhip_imager_flag_dev(gridhip_imager *imager, const double *model, const double *vis, int64_t G,
                            const int64_t *group, const double *wt_in, double nsigma, double amax, int64_t min_count,
                            int64_t niter, double *wt_out, uint8_t *flags_out, double *group_stats, double *stats);

/* ---- time-frequency flagging: SumThreshold and the scale-invariant rank operator over a baseline's waterfall ----------------
 * The reference has no flagging: the semantics are defined here.  gridhip_flag_residuals looks at every sample on its own;
 * interference that lifts every channel of a few time steps, or one channel for a whole scan, by about one sigma shows
 * only in sums along time or frequency.  This is SumThreshold (Offringa et al. 2010) followed by the SIR operator (Offringa
 * et al. 2012), which extends the flags over samples that are mostly surrounded by flags.
 * DATA.  A dense cube of B baselines x T time steps x F channels, n = B T F samples.  order 0: [B][T][F]; order 1:
 *     [T][B][F], the order of a measurement set; F is innermost in both and nothing is copied or transposed for either.
 *     vis: interleaved complex doubles; model_vis: the same shape, or NULL for zero; wt_in: n doubles s_k, or NULL for all
 *     ones.  A cell of the cube that holds no measurement carries the weight 0.
 * CLASSES.  The FIRST class that applies sets the code of a sample in flags_out (n bytes, may be NULL):
 *     1            FLAGGED ON INPUT  s_k is not > 0 (zero, negative, NaN)
 *     3            NOT FINITE        a_k is NaN or Inf
 *     16 + 8 r + k flagged by SumThreshold in round r, stage k
 *     8            added by the SIR operator
 *     0            KEPT
 *     a_k is the amplitude of vis - model_vis exactly as gridhip_flag_residuals defines it: each component one rounded
 *     subtraction, a_k = sqrt(re * re + im * im) with both products rounded, the sum rounded, no fused multiply-add and a
 *     correctly rounded square root.
 * ROUNDS r = 0 .. niter - 1, 0 <= niter <= 4, over the PARTICIPANTS, the samples of class 0.  For every baseline b:
 *     n_b the number of its participants; med_b and MAD_b the lower medians of gridhip_flag_residuals (the element of rank
 *     (n_b - 1) / 2 of a_k, and of |a_k - med_b|); sigma_b = 1.4826 * MAD_b.  If n_b < min_count or sigma_b == 0 the
 *     baseline is not thresholded in this round.  Otherwise e_k = a_k - med_b, one rounded subtraction, and for the STAGES
 *     k = 0 .. K - 1, 1 <= K <= 7, chi_k(b) = levels[k] * sigma_b, one rounded product, with the window length M = 2^k.
 *     levels: K finite positive doubles, in host memory in both forms (they are read while the call is checked).
 * A STAGE works from the participants as the previous stage left them; both directions use the same set.  Along a row of
 *     length L (L = F along frequency, L = T along time) a direction with M > L does nothing.  Otherwise x_i = e_i for a
 *     participant and +0.0 otherwise, c_i = 1 for a participant and 0 otherwise, and the window sums are the doubling tree
 *         S^(1)_j = x_j,   S^(2m)_j = S^(m)_j + S^(m)_{j+m}, each addition rounded once,
 *     C_j likewise (exact), both for the starts j = 0 .. L - M only.  Window j is HIT when C_j > 0 and
 *     S_j > chi_k * (double)C_j, the product rounded once; sample i is hit when any window j in [max(0, i - M + 1),
 *     min(i, L - M)] is hit.  A participant that is hit in either direction gets the code 16 + 8 r + k and is no
 *     participant from the next stage on.  Only positive excess is tested: interference adds power.
 *     A round in which no stage flags anything ends the loop.
 * SIR runs after the rounds, also with niter = 0: along frequency with eta_f, then along time with eta_t on the result; a
 *     direction whose eta == 0 is skipped.  q = rint(eta * 2^20) (the product is exact).  Per row the int64 weights are
 *     w = q for the codes 3, 8 and >= 16, q - 2^20 for code 0, and 0 for code 1 - a missing cell neither attracts nor repels
 *     flags.  P_0 = 0, P_{j+1} = P_j + w_j; a sample x of code 0 gets the code 8 when
 *         max_{j > x} P_j - min_{i <= x} P_i >= 0,
 *     that is when some interval around it holds a fraction of at least (1 - eta) of flagged samples.  Integer arithmetic.
 * OUTPUTS.  wt_out (n doubles; may be wt_in itself) holds s_k (1 without weights) for code 0 and exactly +0.0 otherwise;
 *     vis is never written.  baseline_stats ([B][4] doubles, may be NULL) holds { n_b, med_b, MAD_b, chi_0(b) } as the last
 *     round that ran saw them; a baseline that was not thresholded gives chi_0 = +Inf, an empty one { 0, NaN, NaN, +Inf },
 *     and with niter = 0 every baseline has that form with its count.  stats (8 doubles, may be NULL): { rounds run (the
 *     one that flagged nothing included), participants at the start, flagged by SumThreshold, not finite, added by SIR, 0,
 *     flagged on input, kept }.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context; B, T or F < 1; order not 0 or 1; a
 * NULL vis or wt_out; K outside 1..7 or a NULL levels; a level not finite or <= 0; eta_f or eta_t not in [0, 1);
 * min_count < 1; niter outside 0..4; any output overlapping an input or another output, other than wt_out == wt_in.
 * GRIDHIP_EUNSUPPORTED: B above 2^18, T or F above 2^20 (1048576), n above 2^32 - 1.
 * gridhip_sumthreshold is synchronous and stages host arrays through the context's pool.  The _dev form takes device
 * pointers (levels stays a host array) and enqueues kernels only on the context's stream - no memset node, no copy node;
 * it allocates nothing after the first call of a shape (the scratch - 13 B per sample, 16 B more when a SIR direction runs,
 * 1 KB of bins and 40 B of state per baseline - comes from the context's pool), never synchronises, reads nothing back
 * and can be captured into a graph.  The stop test lives on the device as in gridhip_flag_residuals: all rounds are
 * enqueued, the stages of a round count what they flag, and every launch of the next round reads that count first and
 * returns at once when it is zero.  The launch count, 3 + niter (32 + K) + 2 per SIR direction (2 more for niter = 0),
 * depends on (niter, K, eta) and on nothing in the data.
 * A call is: the front pass and, per round, the select of gridhip_flag_residuals (one copy of each serves both); per stage
 * one launch in which a work-group owns a tile of tile_t x tile_f samples of one baseline (gridhip_sumthreshold_tile),
 * stages x and c of the tile and a halo of M - 1 either side along the direction in LDS, builds the tree and the sliding
 * OR of the hits there by the same doubling, for both directions, and writes the codes of its own tile only, in place;
 * per SIR direction a forward scan with a running minimum and a backward running maximum, one wave per row; and a pass
 * that writes wt_out.
 * DETERMINISM.  Every output is an order statistic, a count, an integer sum or a fixed tree of rounded additions:
 * integer atomics only, no floating-point atomic.  The bits are the same for the host and _dev forms, for two runs, for
 * both orders of the same cube, and for a numpy restatement (S = S[..., :-m] + S[..., m:] is the tree).
 * NOT HERE: the smooth background fit of the full AOFlagger strategy (model_vis, for instance an imager's prediction, is
 * how a caller removes structure); several correlations in one call (call per Stokes plane and combine the weights); an
 * imager form; two-sided thresholds; windows above 64; several devices. */
int gridhip_sumthreshold(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int order, const double *vis,
                         const double *model_vis, const double *wt_in, int64_t K, const double *levels, double eta_f,
                         double eta_t, int64_t min_count, int64_t niter, double *wt_out, uint8_t *flags_out,
                         double *baseline_stats, double *stats);
int gridhip_sumthreshold_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int order, const double *vis,
                             const double *model_vis, const double *wt_in, int64_t K, const double *levels, double eta_f,
                             double eta_t, int64_t min_count, int64_t niter, double *wt_out, uint8_t *flags_out,
                             double *baseline_stats, double *stats);
/* the stage kernel's tile, so that a caller (a test) can stand either side of its edges; GRIDHIP_EINVAL for a NULL */
int gridhip_sumthreshold_tile(int64_t *tile_t, int64_t *tile_f);

/* ---- rotation-measure synthesis: the Faraday dispersion function of every line of sight, and RM-CLEAN ----------------------
 * The reference has no polarisation: the semantics are defined here.  After jonescal -> apply_jones -> stokes -> one imager
 * per Stokes plane -> jclean a caller holds Q and U images per channel.  RM synthesis (Brentjens & de Bruyn 2005) turns the
 * complex polarisation P(lambda^2) = Q + iU of a line of sight into the Faraday dispersion function
 *     F(phi_j) = K sum_c w_c P_c exp(-2 i phi_j (lambda_c^2 - lambda_0^2)),
 * and RM-CLEAN (Heald et al. 2009) deconvolves it with the RM spread function (RMSF), a Hogbom loop along phi.
 * All arrays are doubles; complex arrays are interleaved (re, im).  "Rounded" means one IEEE operation, never contracted
 * into a fused multiply-add, so that numpy reproduces the bits (tests/rm_ref.py restates every rule below).
 * A LINE OF SIGHT (LOS) is one of M flat cells; M is any count, not only N^2: a caller may hand over an image in row
 * slabs and so bound the cube's memory (at N = 2400, J = 400 a whole cube is 36 GB).
 *
 * gridhip_rm_tables(C, J, lam2[C], weights[C] or NULL (all 1), phi0, dphi, fwhm, tables) makes the table the other two
 * read, GRIDHIP_RM_TABLE_DOUBLES(C, J) doubles in four parts:
 *   head[16] = { valid, C, J, phi0, dphi, lam0^2, K, sum w, fwhm, 0 ... }.  sum w and sum w lam2 are plain sums, c ascending
 *       from 0, every product rounded, by one thread; K = 1 / sum w; lam0^2 = (sum w lam2) / sum w.  valid = 1 when every
 *       lam2[c] is finite, every w_c finite and >= 0, sum w finite and > 0 and sum w lam2 finite - judged on the device, by
 *       the prologue kernel; otherwise valid = 0, lam0^2 = K = sum w = 0 and E, R and G are all zeros.
 *       Below a_c = lam2[c] - lam0^2 and kw_c = K * w_c.
 *   E[C][J] complex, j fastest: phi_j = phi0 + j * dphi (the product rounded, then added); t = (phi_j * a_c) * INV_PI with
 *       INV_PI = 0.3183098861837907; r = t - rint(t), exact; (sn, cs) = sincospi(2 r); E = (kw_c * cs, -(kw_c * sn)): the
 *       phasor kw_c exp(-2 i phi_j a_c) with the weight folded in, the phase reduced as the direct-Fourier prediction does.
 *   R[2J - 1] complex, the RMSF at the lags lag_k = (k - (J - 1)) * dphi: R_k = sum_c kw_c exp(-2 i lag_k a_c), every term
 *       formed by the recipe of E with lag_k for phi_j, added with c ascending from (0, 0).  R[J - 1] = (sum kw_c, 0).
 *   G[2J - 1] real, the restoring function: x = lag_k / fwhm, G_k = exp(-(2.772588722239781 * (x * x))) (4 ln 2).
 *   One thread per entry; the only sum is the RMSF's, over at most 1024 channels: a create-once step.
 *   GRIDHIP_EINVAL: C outside 1..1024, J outside 1..512; phi0, dphi or fwhm not finite; dphi or fwhm not > 0; a NULL lam2
 *   or tables; arrays that overlap.
 *
 * gridhip_rmsynth(M, C, J, tables, Q[C][M], U[C][M], cube[J][M] complex, stats[8]): per output element, c ascending from
 *   acc = (0, 0):   acc.re = acc.re + (E.re * q - E.im * u),   acc.im = acc.im + (E.re * u + E.im * q),
 *   every product rounded and the bracket rounded.  A LOS with a non-finite Q or U in any channel gets NaN in all 2J values
 *   and is counted in stats[0].  stats = { bad LOS, 0, 0, 0, 0, 0, 0, invalid }: when the table's head has valid = 0, or its
 *   C or J differ from the arguments, stats = { 0, ..., 0, 1 } and the cube is left as it is (in the host form too).
 *   GRIDHIP_EINVAL: M < 1, C or J out of range, a NULL pointer, a cube that is not 16-byte aligned, arrays that overlap.
 *   GRIDHIP_EUNSUPPORTED: more than 2^31 - 1 tiles of 64 LOS x 64 depths (M above 1.7 x 10^10 at J = 512).
 *   The kernel is a register-tiled product in plain fp64 vector arithmetic (no matrix instruction: v_mfma_f64 fixes its own
 *   summation order and fuses): a work-group owns rm_tile()[0] LOS x rm_tile()[1] depths, stages rm_tile()[2] channels of E,
 *   Q and U at a time in LDS and reads Q and U as the two real cubes they are.  Every output element belongs to one lane,
 *   which adds its channels in order.
 *
 * gridhip_rmclean(M, J, tables, cube[J][M], model[J][M] or NULL, gain, threshold, niter, nsigma, noise (ONE double, or NULL
 *   when nsigma == 0), restore, maps[7][M], stats[8]).  The stop level is L = max(threshold, nsigma * sigma) as
 *   gridhip_clean_auto forms it: L = threshold, and when nsigma > 0, sigma = *noise and L = nsigma * sigma where that is
 *   larger (noise is not read when nsigma == 0); L2 = L * L, rounded once.  nsigma > 0 with a NaN sigma gives stats =
 *   { 0, 0, 0, 0, 0, 0, 1, 0 } and touches nothing else; a table whose head has valid = 0, a C outside 1..1024 or another J
 *   gives stats = { 0, ..., 0, 1 } and touches nothing else (the NaN sigma is reported first).
 *   Per LOS, repeat:
 *     1. p_j = re * re + im * im, each product rounded;
 *     2. k = the depth of the largest p, ties to the lowest j, a NaN never selected (no depth left: p_k = -1, k = -1);
 *     3. p_k <= L2: stop, reason 1 - before anything is subtracted and before the niter test;
 *     4. niter components taken: stop, reason 0;
 *     5. f = (gain * re_k, gain * im_k); model_k += f (the model is accumulated into, never zeroed);
 *     6. for every j, r = R[j - k + J - 1]:  re_j -= (f.re * r.re - f.im * r.im),  im_j -= (f.re * r.im + f.im * r.re),
 *        every product and every bracket rounded.
 *   A LOS with any non-finite value in the cube is left untouched (cube and model): reason 3, 0 iterations, j* = -1 and
 *   NaN in the other maps.  restore = 1 (model must not be NULL), after the loop:
 *     cube_j = residual_j + sum_k model_k * G[j - k + J - 1], k ascending over the depths whose model value is not exactly
 *     (0, 0), each product rounded and added in that order, starting from the residual; model is the whole accumulated
 *     model, what earlier calls left in it included.
 *   maps[.][m] = { iterations, reason, j*, p*, phi_fit, Re F_j*, Im F_j* }: j* and p* by rule 2 on the cube as the call
 *   leaves it (all four are NaN and j* = -1 when no depth can be selected); phi_fit = phi_j* = phi0 + j* * dphi, and if
 *   0 < j* < J - 1 and d = (p_- - p*) + (p_+ - p*) < 0 then off = (0.5 * (p_- - p_+)) / d and phi_fit = phi_j* + off * dphi,
 *   every step rounded (p_-, p_+: the neighbours of j*).
 *   stats = { bad LOS, sum of iterations, LOS stopped by niter, LOS stopped at the level, 0, L, NaN sigma, invalid table }:
 *   counts are integer sums and so free of order.
 *   GRIDHIP_EINVAL: M < 1, J out of range, gain or threshold not finite, niter < 0, nsigma not finite or < 0, nsigma > 0
 *   with a NULL noise, restore not 0 or 1, restore = 1 with a NULL model, a NULL tables, cube, maps or stats, a cube or
 *   model that is not 16-byte aligned, arrays that overlap.  GRIDHIP_EUNSUPPORTED: M above 2^40.
 *   The kernel: one wave per LOS, four consecutive LOS per work-group; depth j in register j / 64 of lane j % 64 (at most 8
 *   complex residuals and 8 model values per lane, all in registers); R and G staged once per work-group in LDS (24 KB);
 *   the arg-max a wave reduction over (p, j) pairs; in the subtraction consecutive lanes read consecutive entries of R; the
 *   restore broadcasts model_k from its lane and skips zeros for the whole wave at once.  The loop's length differs
 *   between waves, never within one.  No floating-point atomic; one integer atomic per wave and counter for the stats.
 *
 * FORMS.  The host forms are synchronous and stage through the context's pool (gridhip_rmclean reads the table's C from
 * its head in host memory to know its size).  The _dev forms take device pointers for EVERY array - lam2, weights and noise
 * too, so nothing needs a copy node - enqueue kernels only on the context's stream (2, 3 and 3 launches), allocate nothing
 * after the first call (64 bytes of counters from the pool), read nothing back, never synchronise and can be captured into a
 * graph.  Both forms run the same kernels and give the same bits, as do two runs, and as does the numpy restatement
 * given the library's table (the table itself agrees within the rounding of sincospi and exp).
 * NOT HERE: per-LOS channel weights or blanked channels (a LOS with a NaN is dropped whole); a fused synthesis and clean
 * that never writes the cube; per-LOS thresholds; multi-scale RM-CLEAN; QU-fitting; derotated angle maps (the caller takes
 * 0.5 atan2(Im, Re) - phi_fit lam0^2); matrix instructions; several devices. */
#define GRIDHIP_RM_MAX_CHANNELS 1024
#define GRIDHIP_RM_MAX_DEPTHS 512
#define GRIDHIP_RM_HEAD 16
#define GRIDHIP_RM_MAPS 7
#define GRIDHIP_RM_STATS 8
#define GRIDHIP_RM_TABLE_DOUBLES(C, J) (16 + 2 * (C) * (J) + 3 * (2 * (J) - 1))
int gridhip_rm_tables(gridhip_ctx *ctx, int64_t C, int64_t J, const double *lam2, const double *weights, double phi0,
                      double dphi, double fwhm, double *tables);
int gridhip_rm_tables_dev(gridhip_ctx *ctx, int64_t C, int64_t J, const double *lam2, const double *weights, double phi0,
                          double dphi, double fwhm, double *tables);
int gridhip_rmsynth(gridhip_ctx *ctx, int64_t M, int64_t C, int64_t J, const double *tables, const double *Q,
                    const double *U, double *cube, double *stats);
int gridhip_rmsynth_dev(gridhip_ctx *ctx, int64_t M, int64_t C, int64_t J, const double *tables, const double *Q,
                        const double *U, double *cube, double *stats);
int gridhip_rmclean(gridhip_ctx *ctx, int64_t M, int64_t J, const double *tables, double *cube, double *model, double gain,
                    double threshold, int64_t niter, double nsigma, const double *noise, int restore, double *maps,
                    double *stats);
int gridhip_rmclean_dev(gridhip_ctx *ctx, int64_t M, int64_t J, const double *tables, double *cube, double *model,
                        double gain, double threshold, int64_t niter, double nsigma, const double *noise, int restore,
                        double *maps, double *stats);
/* out[3] = { LOS per work-group, depths per work-group, channels of a chunk } of the synthesis kernel, so that a caller
 * (a test) can stand either side of its edges; GRIDHIP_EINVAL for a NULL */
int gridhip_rm_tile(int64_t *out);

/* ---- continuum subtraction: a smooth function of frequency fitted to every spectrum, subtracted, and kept ------------------
 * The reference has no such step: the semantics are defined here.  Between continuum and line work lies one operation:
 * fit a polynomial along frequency to the line-free channels of every spectrum, subtract it, keep the fit as the continuum
 * (CASA's uvcontsub / imcontsub, Miriad's uvlin).  In model mode it is also the smooth background fit that
 * gridhip_sumthreshold leaves to its caller: the result is a model_vis.
 * "Rounded" means one IEEE operation, never contracted into a fused multiply-add, so that numpy reproduces the bits
 * (tests/contsub_ref.py restates every rule below).
 * DATA.  R rows (spectra) of C channels, n = R C samples; ncomp 1: real values (images), 2: interleaved complex values
 *     (visibilities).  layout 0: [R][C], the channel innermost - both orders of a gridhip_sumthreshold cube, R = B T;
 *     layout 1: [C][R], the channel outermost - the [C, N, N] cube of gridhip_rmsynth, R = N N.  Nothing is transposed or
 *     copied for either.  wt: NULL for all ones, or one double per sample in the data's layout (not interleaved: one per
 *     complex sample).  x: C doubles, the channel coordinate, for instance (nu - mid) / half.  chan_mask: NULL for all
 *     channels, or C bytes; a byte that is not 0 marks a line-free channel that may enter the fit.
 * BASIS.  Chebyshev polynomials by the rounded recurrence T_0 = 1, T_1 = x, T_{p+1} = (2 * x) * T_p - T_{p-1}, every
 *     product and difference rounded once, for p up to 2 * degree.  The EFFECTIVE channel mask is chan_mask[c] != 0 &&
 *     isfinite(x[c]); a channel whose x is not finite has NaN in `out`, in every row and in both modes: the continuum has
 *     no value there.
 * CLASSES.  The FIRST class that applies sets the code of a sample in `codes` (n bytes in the data's layout, may be NULL):
 *     1       FLAGGED ON INPUT  the weight is not finite or not > 0
 *     3       NOT FINITE        a component of the value is NaN or Inf
 *     2       MASKED            the channel is outside the effective channel mask
 *     16 + i  CLIPPED in round i
 *     0       USED in the final fit
 *     The PARTICIPANTS are the samples of class 0 at that moment.
 * FIT of a row.  The channels are walked in ascending order, one accumulator chain per sum, all from +0.0 - no tree, no
 *     floating-point atomic.  For a participant with weight w (1.0 without weights) and value v:
 *         mu_p = mu_p + w * T_p[c]                                          p = 0 .. 2D
 *         g = w * T_k[c];  b_k.re = b_k.re + g * v.re;  b_k.im likewise     k = 0 .. D
 *     every product and sum rounded once.  The normal matrix follows from the moments by the product identity
 *     T_j T_k = (T_{j+k} + T_{|j-k|}) / 2:   A_jk = 0.5 * (mu_{j+k} + mu_{|j-k|}),   2D + 1 accumulators instead of
 *     (D + 1)(D + 2) / 2.  The solve is LDL^T without pivoting, k = 0 .. D:
 *         t = A_kk;  t = t - (L_kp * L_kp) * d_p  for p = 0 .. k - 1 in this order, each operation rounded.
 *     The pivot is GOOD when A_kk > 0 and t > 1e-12 * A_kk; then d_k = t and for i > k
 *         s = A_ik;  s = s - (L_ip * L_kp) * d_p  for p = 0 .. k - 1;  L_ik = s / d_k.
 *     At the first pivot that is not good the row's degree becomes k - 1 and the factorisation stops: the leading block of
 *     an LDL^T is the factorisation of the lower-degree problem, so the fit falls back instead of failing.  Degree -1: no
 *     usable sample; the continuum of the row is +0.0.  Forward: z_k = b_k;  z_k = z_k - L_kp * z_p, p ascending.  Back,
 *     over the row's degree only, k descending: a_k = z_k / d_k;  a_k = a_k - L_ik * a_i for i = k + 1 .. degree
 *     ascending; a_k = +0.0 above the degree.  The continuum at channel c:  acc = a_0;  acc = acc + a_k * T_k[c], k = 1 .. D
 *     ascending, for both components.
 * CLIP ROUNDS i = 0 .. niter - 1, 0 <= niter <= 4; none when nsigma == 0.  After a fit, over the participants, r = v -
 *     continuum (one rounded subtraction per component), q_c = w * (r.re * r.re + r.im * r.im) (real data: w * (r * r)),
 *     Q their sum in channel order from +0.0, qbar = Q / (double)n_used.  A participant with q_c > (nsigma * nsigma) * qbar
 *     gets the code 16 + i (the square is rounded once, on the host; then one rounded product per row), and the row is
 *     fitted again from the participants that remain.  A row in which a round clips nothing, or whose degree is -1, is
 *     finished.  Every row is independent: there is no global stop test.
 * OUTPUTS.  out has the data's shape and may be `data` itself.  mode 0: v - continuum, one rounded subtraction per component;
 *     mode 1: the continuum itself - at every channel of every row, masked, flagged and clipped ones included.  coeffs (may
 *     be NULL): [R][D+1][ncomp] for layout 0, [D+1][R][ncomp] for layout 1 - coefficient images, plane 0 the continuum
 *     image at x = 0 (for degree 2 and 3: a_0 - a_2).  rowinfo (may be NULL): [R][4] for layout 0, [4][R] for layout 1: { degree used,
 *     samples in the final fit, samples clipped, final qbar }; the final qbar is that of the closing pass, which forms
 *     the residuals anyway, and NaN for a row without a sample.  stats (8 doubles, may be NULL): { rows, rows at full
 *     degree, rows at reduced degree, rows without a fit, samples used, samples clipped, samples not finite, samples
 *     flagged on input }, from integer atomics.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context, data, x or out; R or C < 1; layout
 * or mode not 0 or 1; ncomp not 1 or 2; degree outside 0..3; nsigma negative or not finite; niter outside 0..4; any output
 * overlapping an input or another output, other than out == data.  GRIDHIP_EUNSUPPORTED: C above 4096, R above 2^31 - 1.
 * FORMS.  gridhip_contsub is synchronous and stages host arrays through the context's pool.  In the _dev form every array,
 * x and chan_mask too, lives on the device; it enqueues three launches on the context's stream - a prologue that writes
 * the table of T_p[c] and the effective mask to scratch, the main kernel, the stats - no memset node, no copy node; it
 * allocates nothing after the first call of a shape (64 B per channel and 64 B of counters from the context's pool; n
 * bytes more only when there are clip rounds and codes is NULL), reads nothing back, never synchronises and can be
 * captured into a graph: a linear chain.  In the main kernel a lane owns a row through all passes - moments, solve, per
 * round the residual sum, then clip and moments, then the closing subtraction - so out == data holds by construction: a
 * row's data is written only in its closing pass.  Layout 1 is read straight from global memory, consecutive lanes at
 * consecutive addresses; for layout 0 a work-group owns `rows` rows and streams chunks of `chunk` channels through LDS,
 * loaded along the channel and walked per lane at a padded pitch (gridhip_contsub_tile reports the two).
 * DETERMINISM.  Every floating-point result belongs to one lane and one fixed order: the same bits for the host and _dev
 * forms, for two runs, for a replayed graph, for the two layouts of the same cube, and for the numpy restatement.
 * NOT HERE: median or other robust estimators; fits along time; splines; per-row channel masks other than through wt (a
 * zero weight is the per-row mask); an imager form; several devices; a uv-plane fit for sources far from the phase
 * centre, where the continuum is not smooth in frequency per baseline (gridhip_phase_shift to the source first). */
#define GRIDHIP_CONTSUB_MAX_CHANNELS 4096
#define GRIDHIP_CONTSUB_MAX_DEGREE 3
#define GRIDHIP_CONTSUB_ROWINFO 4
#define GRIDHIP_CONTSUB_STATS 8
int gridhip_contsub(gridhip_ctx *ctx, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
                    const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter, double *out,
                    double *coeffs, double *rowinfo, uint8_t *codes, double *stats);
int gridhip_contsub_dev(gridhip_ctx *ctx, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
                        const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter,
                        double *out, double *coeffs, double *rowinfo, uint8_t *codes, double *stats);
/* out[2] = { rows per work-group, channels per staged chunk } of the layout-0 kernel, so that a caller (a test) can stand
 * either side of its edges; GRIDHIP_EINVAL for a NULL */
int gridhip_contsub_tile(int64_t *out);

/* ---- delay and rate calibration: a fringe search per baseline, an antenna-based fit, and the apply step -------------------
 * The reference has no calibration: the semantics are defined here.  gridhip_gaincal, gridhip_ddcal and gridhip_jonescal
 * solve one complex number per antenna and solution interval; the term before them in every reduction is a per-antenna
 * delay and phase rate (fringe fitting: Schwab & Cotton 1983), whose phase slope across the band or the interval wipes out
 * the averages that gridhip_average, the gain solvers and the gridders form.
 * All arrays are doubles; complex values are interleaved (re, im).  "Rounded" means one IEEE operation, never contracted
 * into a fused multiply-add, as in the RM section (tests/fringe_ref.py restates every rule below).
 * DATA.  The cube is [B][T][F], the order "btf" of gridhip_sumthreshold (gridhip.waterfall_layout builds it and returns
 *     the pairs): vis and the optional model_vis complex, the optional wt one double per sample.  a1[B], a2[B]: the int64
 *     antenna pair (p, q) of a baseline, each in [0, A).  freq[F] in Hz and time[T] in seconds; neither needs to be uniform.
 *     tint: the time steps of a solution interval, 0 meaning T; I = ceil(T / tint) intervals, the last may be short.
 * MODEL.  V[b,t,f] ~ M[b,t,f] exp(i (psi_p - psi_q)),  psi_a(t,f) = arg g[i,a] + 2 pi tau[i,a] (nu_f - nu0) + 2 pi r[i,a]
 *     (t - tref_i), with nu0 = freq[0] + 0.5 * (freq[F-1] - freq[0]) and tref_i formed the same way from the first and the
 *     last time of interval i.  A solution `sol` is [I][A][4] = { tau, r, Re g, Im g } with |g| = 1: phasors, not angles -
 *     no atan2 enters it.
 * PHASOR RECIPE.  ph(a, b) = exp(2 pi i a b): the turns x = a * b (rounded), r = x - rint(x) (exact), (sn, cs) =
 *     sincospi(2 r), ph = (cs, sn) - the reduction of the RM table's E.  Complex products: x conj(c) = (x.re c.re + x.im c.im,
 *     x.im c.re - x.re c.im) and x c = (x.re c.re - x.im c.im, x.re c.im + x.im c.re), four rounded products and two rounded
 *     sums each; acc + e x as gridhip_rmsynth adds it: acc.re = acc.re + (e.re x.re - e.im x.im), acc.im = acc.im + (e.re x.im
 *     + e.im x.re), every product and the bracket rounded.
 *
 * gridhip_fringe_tables(F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables) makes the table the others read,
 * GRIDHIP_FRINGE_TABLE_DOUBLES(F, T, Nd, Nr) doubles:
 *   head[16] = { valid, F, T, tint (after the 0 -> T rule), I, Nd, Nr, tau0, dtau, r0, drate, nu0, 0 ... }
 *   Ef[F][Nd] complex, j fastest: conj ph(tau_j, a_f), tau_j = tau0 + j * dtau (the product rounded, then added), a_f =
 *       freq[f] - nu0: exp(-2 pi i tau_j (nu_f - nu0)) = (cs, -sn)
 *   Et[T][Nr] complex, k fastest: conj ph(r_k, dt_t), r_k = r0 + k * drate, dt_t = time[t] - tref_i(t)
 *   tref[T]: the I reference times, then zeros;  a[F] = a_f;  dt[T] = dt_t (what the derotation and the apply step read)
 *   valid is judged on the device (one work-group scans freq and time): every freq and time, tau0, dtau, r0, drate and nu0 finite, dtau > 0 and drate > 0;
 *   otherwise valid = 0 and everything behind the head is zeros.  One thread per entry.
 *   GRIDHIP_EINVAL: F outside 1..1024, Nd outside 1..4096, Nr outside 1..1024, T < 1, tint < 0 or above 256 after the
 *   0 -> T rule, a NULL pointer, arrays that overlap.  GRIDHIP_EUNSUPPORTED: T above 2^20.
 *
 * gridhip_fringe_search(B, T, F, A, I, tables, vis, model_vis or NULL, wt or NULL, a1, a2, sol or NULL, j0, j1, k0, k1,
 * peaks[B][I][12], stats[8]) - the hot path.  I is the table's number of intervals, by which the caller has sized peaks and
 *   sol: the call cannot read it from a table on the device, and refuses a table whose head says otherwise.  Per sample, s = wt (1 without), X = (s re V, s im V) conj(M) by
 *   gridhip_gaincal's rounded formula; without a model X = (s re V, s im V).
 *     FLAGGED   a sample whose s is not > 0: selected out, it contributes exactly nothing even when it is NaN
 *     BAD       a (baseline, interval) with an unflagged sample whose X' is not finite
 *   With sol the sample is derotated, X' = ((X conj(d_b)) conj(Df[f])) conj(Dt[t]) in this order, with d_b = g_p conj(g_q)
 *   (the x conj(c) rule), Df[f] = ph(tau_p - tau_q, a_f) and Dt[t] = ph(r_p - r_q, dt_t), made once per (baseline,
 *   interval); without sol X' = X, no product.  Then for j in [j0, j1) and k in [k0, k1):
 *     1. Y[t][j] = sum_f Ef[f][j] X'[t][f], f ascending from (0, 0) by the acc + e x rule (flagged samples add (0, 0));
 *     2. S[j][k] = sum_t Et[t][k] Y[t][j], t ascending over the interval, the same rule;
 *     3. P = re * re + im * im.
 *   The peak (j*, k*) is the largest P, ties to the lowest j, then the lowest k; a NaN is never selected.  Refinement is
 *   gridhip_rmclean's parabola rule on each axis separately: tau_b = tau_j*, and if j0 < j* < j1 - 1 and d = (P_- - P*) +
 *   (P_+ - P*) < 0 then tau_b = tau_j* + ((0.5 * (P_- - P_+)) / d) * dtau (P_-, P_+ at j* -+ 1 and k*); r_b likewise along k.
 *   Energy: e_t = sum_f (re * re + im * im) of the unflagged X', f ascending; N = sum_t e_t, t ascending; n_used the number
 *   of unflagged samples.  coh2 = P* / ((double)n_used * N), 0 when N is not > 0;  z = (Re S* / sqrt(P*), Im S* / sqrt(P*)),
 *   (1, 0) when P* is not > 0.
 *   peaks row = { j*, k*, P*, tau_b, r_b, Re z, Im z, coh2, n_used, N, code, 0 };  code, the first that applies:
 *     3  p == q or an antenna out of range     1  empty: no unflagged sample     2  BAD     0  ok
 *   A row whose code is not 0 is { -1, -1, 0, 0, 0, 1, 0, 0, n_used, 0, code, 0 }.  An all-zero baseline is ok: the tie
 *   goes to (j0, k0), coh2 = 0.
 *   stats = { flagged samples, BAD, empty, refused (code 3), ok rows, 0, 0, invalid }: when the table's head has valid = 0,
 *   its F, T or I differ from the arguments, or the cells do not lie in its grid, stats = { 0, ..., 0, 1 } and peaks is left as
 *   it is (in the host form too).
 *   GRIDHIP_EINVAL: B, T < 1, F outside 1..1024, A < 2, I outside 1..T, cells not 0 <= j0 < j1 <= 4096, 0 <= k0 < k1 <= 1024, a NULL
 *   tables, vis, a1, a2, peaks or stats, a vis or model_vis that is not 16-byte aligned, an output overlapping an input or
 *   the other output.  GRIDHIP_EUNSUPPORTED: B above 2^24, T above 2^20, A above 1024, B T above 2^31 - 1.
 *   The kernels.  A work-group owns a baseline and fringe_tile()[0] delays and walks the intervals: X' and Ef stream through
 *   LDS in chunks of fringe_tile()[1] channels, Y[t][j] is accumulated in registers, one output element per lane-slot,
 *   channels in order; Y is parked in LDS and S formed against Et, fringe_tile()[2] rates per lane-pass, t in order, with a
 *   running (P, j, k) maximum per lane, reduced by the tie rule into one candidate per tile.  A second kernel, one wave per
 *   (baseline, interval), takes the best tile in ascending order, recomputes the five values the parabolas need by the same
 *   two ordered sums - so the bits do not depend on the tile borders - and forms the energy and the row.  No matrix
 *   instruction (gridhip_rmsynth's argument); 53 KB of LDS per work-group; integer atomics only, for the stats.
 *
 * gridhip_fringe_solve(B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info[I][A], stats[8]).
 *   The baseline weight w_b = coh2 when code == 0, n_used >= min_count, coh2 >= min_coh2, coh2 > 0, the row's tau_b, r_b, z
 *   and coh2 are finite and the pair is in range with p != q; else 0 and the baseline is not USED.  Per interval three
 *   antenna-based problems are solved together from x_tau = x_r = 0, h = (1, 0); sweep it = 0, 1, ..., for every antenna a
 *   that a used baseline touches, b ascending over the used baselines that touch it, all sums from +0.0:
 *       wz = (w_b * Re z_b, w_b * Im z_b);  den = den + w_b
 *       p_b = a:  nt = nt + w_b * (tau_b + x_tau[q]);  nr likewise;  num = num + wz h[q]        (the acc + e x rule)
 *       q_b = a:  nt = nt + w_b * (x_tau[p] - tau_b);  nr likewise;  num = num + conj(wz) h[p]  (num.re + (wz.re h.re +
 *                 wz.im h.im), num.im + (wz.re h.im - wz.im h.re))
 *       x_tau' = nt / den;  x_r' = nr / den;  m = num.re * num.re + num.im * num.im;  h' = (num.re / sqrt(m), num.im /
 *       sqrt(m)) when m > 0 and finite, else h
 *       on odd it: x' <- 0.5 * (x' + x) for both, and h' <- the sum 0.5 * (h' + h) per component, divided by its sqrt(re * re +
 *       im * im) when that is > 0 and finite, else h
 *   (Jacobi: every antenna reads the values of the sweep before.)  An antenna no used baseline touches keeps its values and
 *   is UNSOLVED.  Stop after the sweep in which c_tau <= tol * s_tau, c_r <= tol * s_r and c_h <= tol, with c = the largest
 *   |x' - x| and s = the largest |x'| over the antennas of the interval, c_h the largest sqrt(dre * dre + dim * dim).
 *   Then, if refant >= 0 and it is solved: x_tau and x_r of every solved antenna minus refant's, h <- h conj(h_refant), and
 *   h_refant = (1, 0); an interval whose refant is unsolved stays unreferenced and is counted.  Then sol is accumulated
 *   into, for the solved antennas only: tau += x_tau, r += x_r, g <- g h (the x c rule) divided by its sqrt(re * re + im * im)
 *   when that is > 0 and finite.  info[i][a] = the used baselines that touch a; 0: unsolved.
 *   stats = { sweeps (the most of any interval), used baselines, unsolved antennas, unreferenced intervals, rms_tau, rms_r,
 *   0, 0 }: rms = sqrt(sum w y^2 / sum w) over the used baselines with y = tau_b or r_b (0 without any) - a thread adds
 *   ceil(B / 256) consecutive baselines from +0.0, w * (y * y), then the 256 runs are added in order, then the intervals.
 *   No floating-point atomic: the same bits on every run.  One work-group per interval; a thread owns an antenna.  The
 *   baselines pass through LDS twice, 256 at a time - once to count, once to fill - which leaves every antenna a list of
 *   its used baselines in ascending order (96 B of pooled scratch per baseline and interval); a sweep reads only those.
 *   Measured on a numpy prototype: 50 sweeps reach 1e-16 on a full array of 8 or 32 antennas; a pure
 *   chain of 32 antennas does not converge in 200 - Jacobi needs a well-connected array.
 *   GRIDHIP_EINVAL: B or I < 1, A < 2, min_count or min_coh2 negative or not finite, refant >= A (negative: none), niter
 *   outside 0..100000, tol negative or not finite, a NULL pointer, arrays that overlap.  GRIDHIP_EUNSUPPORTED: A above 1024,
 *   B above 2^24, I above 2^20.
 *
 * gridhip_fringefit(B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count, min_coh2, refant,
 * niter, tol, warm, sol, peaks, info, stats) is the driver; I, Nd and Nr are the table's (it cannot read them from the
 *   device).  warm = 0: sol starts as { 0, 0, 1, 0 }.  Round 0 searches the whole grid, derotating by sol when warm; the
 *   rounds 1 .. rounds - 1 (rounds in 1..4) derotate by the current sol and search only the cells within (wj, wk) of the grid's
 *   zero, jz = rint(-tau0 / dtau) and kz = rint(-r0 / drate) clamped into the grid: [jz - wj, jz + wj] x [kz - wk, kz + wk],
 *   cut at the grid's edges.  Every search is followed by gridhip_fringe_solve, which accumulates into sol.  It returns sol,
 *   the last round's peaks (residual delays and rates against sol BEFORE that round's solve) and info, and stats = { sweeps
 *   of the last solve, flagged samples, BAD, empty, unsolved antennas, rms_tau / dtau, rms_r / drate (the last round's, in
 *   cells), invalid }; invalid = 1 (a head that does not fit F, T, I, Nd, Nr): nothing else is meaningful, and no solve ran.
 *   A fixed number of launches (6 per round, 1 or 2 more), nothing read back, the stop test on the device: the _dev form
 *   can be captured.  GRIDHIP_EINVAL / EUNSUPPORTED: those of the search and the solve; I outside 1..T, Nd, Nr out of range,
 *   rounds outside 1..4, wj outside 0..4096, wk outside 0..1024, warm not 0 or 1.
 *
 * gridhip_apply_fringe(B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in or NULL, vis_out, wt_out or NULL) reads only
 *   the head, a[F] and dt[T] of a table (any Nd, Nr).  D = d_b, Df[f], Dt[t] as in the search.  inverse 1 (correct data):
 *   vis_out = ((vis_in conj(d_b)) conj(Df[f])) conj(Dt[t]); inverse 0 (corrupt a model): vis_out = ((vis_in d_b) Df[f])
 *   Dt[t].  Weights are copied (ones without wt_in).  A sample that touches an antenna whose sol row is not finite, or an
 *   antenna out of range, keeps its value and gets the weight +0.0 (gridhip_apply_gains' rule).  In place (vis_out ==
 *   vis_in, wt_out == wt_in) is allowed; any other overlap is refused.  A head that does not fit F, T and I: nothing is
 *   written.  GRIDHIP_EINVAL: the cube's limits as above, I outside 1..T, a NULL tables, sol, a1, a2, vis_in or vis_out, inverse not 0 or 1,
 *   a cube that is not 16-byte aligned, overlap.
 *
 * FORMS.  The host forms are synchronous, stage through the context's pool and read the table's head in host memory to know
 * the table's size.  The _dev forms take device pointers for EVERY array, enqueue kernels only on the context's stream, read
 * nothing back, never synchronise and can be captured.  Every call that sizes an array by I takes I from its caller and the
 * kernels compare it with the table's head.  Both forms run the same kernels and give the same bits, as do two runs and the
 * numpy restatement given the library's table.
 * NOT HERE: the order "tbf"; rates that scale with frequency; multi-band delays; a global least-squares polish over all
 * samples; an imager form; several devices.  Dispersive (TEC) delays: the next section, "dispersive delay (TEC)
 * calibration". */
#define GRIDHIP_FRINGE_MAX_CHANNELS 1024
#define GRIDHIP_FRINGE_MAX_DELAYS 4096
#define GRIDHIP_FRINGE_MAX_TINT 256
#define GRIDHIP_FRINGE_MAX_RATES 1024
#define GRIDHIP_FRINGE_MAX_ANTENNAS 1024
#define GRIDHIP_FRINGE_MAX_ITER 100000
#define GRIDHIP_FRINGE_MAX_ROUNDS 4
#define GRIDHIP_FRINGE_HEAD 16
#define GRIDHIP_FRINGE_PEAK 12
#define GRIDHIP_FRINGE_STATS 8
#define GRIDHIP_FRINGE_TABLE_DOUBLES(F, T, Nd, Nr) (16 + 2 * (F) * (Nd) + 2 * (T) * (Nr) + 2 * (T) + (F))
int gridhip_fringe_tables(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, const double *time,
                          double tau0, double dtau, int64_t Nd, double r0, double drate, int64_t Nr, double *tables);
int gridhip_fringe_tables_dev(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, const double *time,
                              double tau0, double dtau, int64_t Nd, double r0, double drate, int64_t Nr, double *tables);
int gridhip_fringe_search(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                          const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                          const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1, double *peaks, double *stats);
int gridhip_fringe_search_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                              const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                              const int64_t *a2, const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1,
                              double *peaks, double *stats);
int gridhip_fringe_solve(gridhip_ctx *ctx, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                         const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter, double tol,
                         double *sol, double *info, double *stats);
int gridhip_fringe_solve_dev(gridhip_ctx *ctx, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                             const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter,
                             double tol, double *sol, double *info, double *stats);
int gridhip_fringefit(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                      const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                      const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count, double min_coh2,
                      int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                      double *stats);
int gridhip_fringefit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                          const double *tables, const double *vis, const double *model_vis, const double *wt,
                          const int64_t *a1, const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count,
                          double min_coh2, int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks,
                          double *info, double *stats);
int gridhip_apply_fringe(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                         const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                         const double *wt_in, double *vis_out, double *wt_out);
int gridhip_apply_fringe_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                             const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                             const double *wt_in, double *vis_out, double *wt_out);
/* out[3] = { delays per work-group, channels per staged chunk, rates per lane-pass } of the search kernel, so that a caller
 * (a test) can stand either side of its edges; GRIDHIP_EINVAL for a NULL */
int gridhip_fringe_tile(int64_t *out);

/* ---- dispersive delay (TEC) calibration: a delay-TEC search per baseline, the fringe section's antenna fit, the apply step --
 * The reference has no calibration: the semantics are defined here.  Below about 350 MHz the ionosphere puts a phase of
 * -2 pi kappa dTEC / nu on every antenna, dTEC the differential total electron content in TEC units (1e16 electrons / m^2)
 * and kappa = GRIDHIP_TEC_KAPPA = e^2 1e16 / (8 pi^2 eps0 m_e c) = 1.3445365934456e9 turns Hz per TEC unit (CODATA 2018;
 * 2 pi kappa = 8.448e9 rad Hz).  That phase curves across the band: the linear delay of the section before cannot absorb it.
 * This section inherits from "delay and rate calibration", by name: DATA, the PHASOR RECIPE with the x conj(c), x c and
 * acc + e x rules, FLAGGED and BAD, the row of peaks, and the FORMS paragraph (tests/tec_ref.py restates every rule below).
 * MODEL, per solution interval i:  psi_a(f) = arg g[i,a] + 2 pi tau[i,a] a_f + 2 pi tec[i,a] c_f, with
 *     a_f = freq[f] - nu0, nu0 as in the fringe section;
 *     z_f = -(kappa * (1 / freq[f] - 1 / nu0)), every operation rounded: the dispersive coordinate, 0 at nu0;
 *     s   = (sum_f a_f * z_f) / (sum_f a_f * a_f), the products rounded, both sums f ascending from +0.0; s = 0 when the
 *           denominator is not > 0;
 *     c_f = z_f - s * a_f (the product rounded): z with its linear part taken out, sum_f a_f c_f = 0 to rounding.
 *   THE TEC AXIS IS THE ORTHOGONALISED ONE.  Along the raw z_f the delay and TEC axes are almost collinear and the per-axis
 *   parabola with windowed later rounds stalls on the ridge; along c_f it converges by a factor of about
 *   12 per round.  The delay this section reports is therefore the EFFECTIVE delay tau_eff = tau_clock + s * tec, and the
 *   table carries s so that a caller can separate the clock: tau_clock = tau - s * tec (gridhip.tec_clock).
 *   A solution `sol` is [I][A][4] = { tau, tec, Re g, Im g } with |g| = 1.  There is no time axis: a step only selects its
 *   interval.
 *
 * gridhip_tec_tables(F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables) makes the table the others read,
 * GRIDHIP_TEC_TABLE_DOUBLES(F, Nd, Nm) doubles.  It takes no time array.
 *   head[16] = { valid, F, T, tint (after the 0 -> T rule), I, Nd, Nm, tau0, dtau, tec0, dtec, nu0, s, kappa, 0, 0 }
 *   Ef[F][Nd] complex, j fastest: conj ph(tau_j, a_f), tau_j = tau0 + j * dtau, as in the fringe table
 *   Em[F][Nm] complex, m fastest: conj ph(tec_m, c_f), tec_m = tec0 + m * dtec (the product rounded, then added)
 *   a[F] = a_f;  c[F] = c_f (what the derotation and the apply step read)
 *   valid is judged on the device by one work-group: every freq finite and > 0, tau0, dtau, tec0, dtec, nu0 and s finite,
 *   dtau > 0 and dtec > 0; otherwise valid = 0, nu0 = s = 0 and everything behind the head is zeros.
 *   GRIDHIP_EINVAL: F outside 1..1024, Nd outside 1..4096, Nm outside 1..1024, T < 1, tint outside 0..T (0: T; there is no
 *   cap of 256 - time is summed before the search), a NULL pointer, arrays that overlap.  GRIDHIP_EUNSUPPORTED: T above 2^20.
 *
 * gridhip_tec_search(B, T, F, A, I, tables, vis, model_vis or NULL, wt or NULL, a1, a2, sol or NULL, j0, j1, m0, m1,
 * peaks[B][I][12], stats[8]) - the hot path.  I is the table's, as in the fringe search.
 *   1. Per sample X as in the fringe search.  With sol: d_b = g_p conj(g_q) (the x conj(c) rule) and Dfm[f] = ph(tau_p -
 *      tau_q, a_f) ph(tec_p - tec_q, c_f) (the x c rule, the delay phasor first), made once per (baseline, interval);
 *      X' = (X conj(d_b)) conj(Dfm[f]).  Without sol X' = X, no product.
 *   2. Xbar[f] = sum_t X'[t][f], t ascending over the interval from (0, 0), plain rounded sums per component; a flagged
 *      sample adds (0, 0).
 *   3. S[j][m] = sum_f Ef[f][j] (Em[f][m] Xbar[f]) for j in [j0, j1), m in [m0, m1): the inner product by the x c rule with
 *      x = Em and c = Xbar, then the acc + e x rule with e = Ef, f ascending from (0, 0).  P = re * re + im * im.
 *   4. The peak (j*, m*) is the largest P, ties to the lowest j, then the lowest m; a NaN is never selected.  The fringe
 *      section's parabola per axis where the peak is interior: tau_b along j at m*, tec_b along m at j*.
 *   5. Energy N (of the unflagged X' per sample: e_t = sum_f, then N = sum_t), n_used, coh2 = P* / (n_used N), z, the codes
 *      and stats are exactly the fringe search's.
 *   peaks row = { j*, m*, P*, tau_b, tec_b, Re z, Im z, coh2, n_used, N, code, 0 }; a row whose code is not 0 is the fringe
 *   search's.  An all-zero baseline is ok: the tie goes to (j0, m0), coh2 = 0.  stats[7] = 1 and peaks left as it is when
 *   the head has valid = 0, its F, T or I differ from the arguments, or the cells do not lie in its grid.
 *   GRIDHIP_EINVAL: B, T < 1, F outside 1..1024, A < 2, I outside 1..T, cells not 0 <= j0 < j1 <= 4096, 0 <= m0 < m1 <= 1024,
 *   a NULL tables, vis, a1, a2, peaks or stats, a vis or model_vis that is not 16-byte aligned, an output overlapping an
 *   input or the other output.  GRIDHIP_EUNSUPPORTED: B above 2^24, T above 2^20, A above 1024, B T above 2^31 - 1, more
 *   than 2^31 - 1 tiles.
 *   The kernels.  A work-group owns one (baseline, interval) and a tile of tec_tile()[0] delays x tec_tile()[1] TEC cells.
 *   It forms Xbar once in LDS (16 KB), the sample rows read coalesced along f and derotated on the way, and stages Ef and
 *   Em through LDS in chunks of tec_tile()[2] channels (a tile of fewer delays stages as many more channels at a time as
 *   its narrower rows leave room for, up to 32: the sums and their order are the same).  A lane keeps two delays x the tile's TEC cells (1, 2, 4 or 8: a
 *   grid of three TEC cells does not pay for eight) in registers, so one Em Xbar product feeds both delays and one Ef entry
 *   every TEC cell; each accumulator adds its channels in order, unfused.  One candidate per tile.  A second kernel, one wave
 *   per (baseline, interval), takes the best candidate, recomputes the five powers the parabolas need by the same ordered
 *   sums - the bits do not depend on the tile borders - and forms the energy and the row.  No matrix instruction
 *   (gridhip_rmsynth's argument); 52 KB of LDS per work-group; integer atomics only, for the stats.
 *
 * THE ANTENNA FIT IS gridhip_fringe_solve, UNCHANGED.  The delay and TEC values sit in the slots of the row the fringe solve
 *   reads as delay and rate, and it treats the two identically, as linear differences tau_p - tau_q and tec_p - tec_q: there
 *   is no second solver.  Its stats name rms_r what is rms_tec here.
 *
 * gridhip_tecfit(B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count, min_coh2, refant,
 * niter, tol, warm, sol, peaks, info, stats) is the driver: gridhip_fringefit's argument list and stats with Nm for Nr, wm
 *   for wk, and rms_tec / dtec in place of the rate entry.  Round 0 searches the whole grid (derotating by sol when warm);
 *   the rounds 1 .. rounds - 1 (rounds in 1..4) derotate by the current sol and search the cells within (wj, wm) of the grid's
 *   zero, jz = rint(-tau0 / dtau) and mz = rint(-tec0 / dtec) clamped into the grid.  Every search is followed by
 *   gridhip_fringe_solve's kernels, which accumulate into sol.  stats = { sweeps of the last solve, flagged samples, BAD,
 *   empty, unsolved antennas, rms_tau / dtau, rms_tec / dtec, invalid }.  A fixed number of launches (6 per round, 1 or 2
 *   more), nothing read back: the _dev form can be captured.  GRIDHIP_EINVAL / EUNSUPPORTED: those of the search and the
 *   solve; I outside 1..T, Nd, Nm out of range, rounds outside 1..4, wj outside 0..4096, wm outside 0..1024, warm not 0 or 1.
 *
 * gridhip_apply_tec(B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in or NULL, vis_out, wt_out or NULL) follows
 *   gridhip_apply_fringe's rules - the weight copy, +0.0 for a non-finite row or an antenna out of range, in place allowed,
 *   a head that does not fit F, T and I leaves the outputs unwritten - and reads only the head, a[F] and c[F] of a table
 *   (any Nd, Nm).  The phasor is D = d_b Dfm[f]: inverse 1, vis_out = (vis_in conj(d_b)) conj(Dfm[f]); inverse 0,
 *   vis_out = (vis_in d_b) Dfm[f].  GRIDHIP_EINVAL / EUNSUPPORTED: those of gridhip_apply_fringe.
 *
 * NOT HERE: a joint rate axis (run gridhip_fringefit for the rates first); the order "tbf"; higher-order ionospheric terms;
 * Faraday rotation; a direction-dependent TEC screen; an imager form; several devices. */
#define GRIDHIP_TEC_KAPPA 1.3445365934456e9
#define GRIDHIP_TEC_MAX_CHANNELS 1024
#define GRIDHIP_TEC_MAX_DELAYS 4096
#define GRIDHIP_TEC_MAX_CELLS 1024
#define GRIDHIP_TEC_MAX_ROUNDS 4
#define GRIDHIP_TEC_HEAD 16
#define GRIDHIP_TEC_PEAK 12
#define GRIDHIP_TEC_STATS 8
#define GRIDHIP_TEC_TABLE_DOUBLES(F, Nd, Nm) (16 + 2 * (F) * (Nd) + 2 * (F) * (Nm) + 2 * (F))
int gridhip_tec_tables(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, double tau0, double dtau,
                       int64_t Nd, double tec0, double dtec, int64_t Nm, double *tables);
int gridhip_tec_tables_dev(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, double tau0, double dtau,
                           int64_t Nd, double tec0, double dtec, int64_t Nm, double *tables);
int gridhip_tec_search(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                       const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                       const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats);
int gridhip_tec_search_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                           const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                           const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats);
int gridhip_tecfit(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
                   const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                   const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2, int64_t refant,
                   int64_t niter, double tol, int warm, double *sol, double *peaks, double *info, double *stats);
int gridhip_tecfit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
                       const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                       const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2,
                       int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                       double *stats);
int gridhip_apply_tec(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                      const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                      const double *wt_in, double *vis_out, double *wt_out);
int gridhip_apply_tec_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                          const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                          const double *wt_in, double *vis_out, double *wt_out);
/* out[3] = { delays per work-group tile, TEC cells per tile, channels per staged chunk } of the search kernel, so that a
 * caller (a test) can stand either side of its edges; GRIDHIP_EINVAL for a NULL */
int gridhip_tec_tile(int64_t *out);

/* ---- direct-Fourier prediction of a sky-model component list, and a model image as such a list ----------------------------
 * The reference has no such function: the semantics are defined here.  Every other prediction goes through a model image
 * and a degridder; this one evaluates the measurement equation itself,
 *     V(u,v,w) = sum_c S_c(x) E_c(u,v) exp(-2 pi i (u l_c + v m_c + w (n_c - 1))),
 * for a catalogue, for a source outside the imaged field, or as the exact model a calibration solves against.
 * COMPONENTS  comps is [C][GRIDHIP_COMP_DOUBLES = 10] doubles, one row per component:
 *                 { l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0 }
 *     l, m      direction cosines relative to the phase centre.  The pixel [y][x] of an N x N image, N =
 *               gridhip_image_size(theta, lam), lies at l = theta (x - N/2) / N, m = theta (y - N/2) / N with the integer
 *               N/2 (the product first, then the quotient); with this the DFT at an integer cell (u, v) = (i, j) / theta
 *               equals fft_c(model)[N/2 + j][N/2 + i], gridhip_predict's simple kind, for even and odd N
 *     flux      S(x) = f0 + x (f1 + x (f2 + x f3)) by Horner with every product rounded; x is per visibility, (nu - nu_0) /
 *               nu_0 as gridhip_imager_set_spectral_dev takes it.  T in 1..4 says how many f are read: f_T .. f3 are
 *               ignored (taken as 0).  x == NULL means x = 0: only f0 counts, though f0 .. f_{T-1} are still read and must
 *               be finite.
 *     shape     bmaj == 0 && bmin == 0: a point, E = 1 and no exp is evaluated.  Otherwise an elliptical Gaussian with
 *               FWHM axes bmaj >= bmin >= 0 in direction-cosine units and position angle bpa in radians from +m towards +l:
 *                   E = exp(-(pi^2 / (4 ln 2)) (bmaj^2 up^2 + bmin^2 vp^2)),  up = u sin bpa + v cos bpa,
 *                                                                           vp = u cos bpa - v sin bpa
 *               (evaluated as a quadratic form quu u^2 + quv u v + qvv v^2 whose coefficients are formed once per call).
 *               The tenth double is reserved and not read.
 *     n - 1     = -r2 / (1 + sqrt(1 - r2)), r2 = l^2 + m^2: the subtraction form cancels.
 *     SIGN      the phase is -2 pi (u l + v m + w (n - 1)): the minus sign of the forward transform, and w (n - 1) as the
 *               far field of gridhip_w_kernel, exp(+2 pi i w (1 - n)), which a prediction sees unconjugated.
 *     phase     formed in turns: p = u l + v m + w (n - 1) in fp64, r = p - rint(p), which is exact, then the sine and
 *               cosine of 2 pi r with |r| <= 1/2.  fp64 throughout.  With |p| <= 1e4 turns the error of a visibility is
 *               below 1e-10 sum_c |S_c|.
 *     SKIPPED   a component contributes exactly nothing and is counted when any of l, m, f0 .. f_{T-1}, bmaj, bmin, bpa is
 *               not finite, r2 > 1, bmaj < bmin or bmin < 0, or when the quadratic form of its Gaussian is not finite
 *               in fp64: an axis whose square overflows, bmaj above about 1e154.
 * VISIBILITIES  u, v, w in wavelengths with uv_stride as everywhere else, un-mirrored; w == NULL means w = 0; x: n doubles
 *     or NULL.  A visibility with a non-finite u, v or w, or a non-finite x when x is given, predicts exactly 0 and is
 *     counted.  vis_out = pred, or vis_sub - pred (the residual) when vis_sub != NULL - vis_sub[k] itself for such a
 *     visibility.  vis_out == vis_sub is allowed.  vis_out is overwritten, never accumulated.
 * count_dev   a device int64 (the host form: a host int64), or NULL.  When given, the call uses min(max(*count_dev, 0), C)
 *     components and reads no row after them, so a list built on the device - gridhip_components_from_image_dev's - is
 *     predicted with nothing read back.
 * stats       optional, 4 doubles { components used, components skipped, visibilities with non-finite coordinates, the
 *     slices S }.
 * DETERMINISM.  For a given (n, C, options) the result has the same bits on every run: each visibility's sum runs over the
 *     components in list order in one thread, with no atomics in the sum.  When n is too small to fill the device the list
 *     is cut into S slices of ceil(C / S) components (S a function of n and C alone, or the option "dft_slices"), whose
 *     partial sums are added in slice order; S changes the rounding of the sum, not its reproducibility.
 * FROM A MODEL IMAGE.  gridhip_components_from_image turns model[T][N][N] (T Taylor-term planes as gridhip_mfclean leaves
 *     them; T = 1: the model of clean or msclean) into a list: every cell where some term is not zero (a NaN is not zero)
 *     becomes a point component - its l, m by the rule above, f_t the cell's terms, the unused f and the shape fields 0 -
 *     in row-major order, by an ordered compaction (per-segment counts, an exclusive scan, a scatter): the same list on
 *     every run.  *count receives the number found even when it exceeds max_c; only the first max_c rows are written, and
 *     the rows after the last one written are left as they were.  In the _dev form count is a device int64.
 * All arguments are checked before anything is touched, GRIDHIP_EINVAL: a NULL context; n < 0; C < 0; T outside 1..4; a
 * NULL comps with C > 0 (max_c > 0); a NULL u, v or vis_out with n > 0; uv_stride < 1; vis_out overlapping anything but
 * vis_sub (and then only as vis_sub itself); stats overlapping any other argument; max_c < 0; a NULL model or count; an image size below 1; comps, count and
 * model overlapping.  n of 2^31 - 256 or more and N above 2^20 are GRIDHIP_EUNSUPPORTED.  A refused call leaves its outputs
 * unchanged.  n = 0 and C = 0 are valid: with C = 0 vis_out is 0, or vis_sub.
 * The host forms are synchronous and stage through the context's pool.  The _dev forms take device pointers and enqueue
 * kernels only on the context's stream - no memset node, no copy node; they allocate nothing after the first call of a
 * shape (80 B of scratch per component, 16 S B per visibility when S > 1), never synchronise and read nothing back, so
 * they can be captured into a graph.
 * A prediction is: a pass that validates the components and converts each to { l, m, n - 1, f0 .. f3, quu, quv, qvv }; the
 * main kernel, whose work-groups of 256 threads take 512 visibilities each - two per thread, in registers with their two
 * complex sums - and stage the converted components through LDS in chunks of 256 (20 KB), every lane of a wave reading the
 * same component; with S > 1 an epilogue that adds the partial sums and applies vis_sub. */
#define GRIDHIP_COMP_DOUBLES 10
int gridhip_dft_predict(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count, int T, int64_t n,
                        const double *u, const double *v, const double *w, int64_t uv_stride, const double *x,
                        const double *vis_sub, double *vis_out, double *stats);
int gridhip_dft_predict_dev(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count_dev, int T, int64_t n,
                            const double *u, const double *v, const double *w, int64_t uv_stride, const double *x,
                            const double *vis_sub, double *vis_out, double *stats);
int gridhip_components_from_image(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model, int64_t max_c,
                                  double *comps, int64_t *count);
int gridhip_components_from_image_dev(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model,
                                      int64_t max_c, double *comps, int64_t *count);

/* ---- source finding: from a restored map to a list of Gaussian components, on the device -----------------------------------
 * The reference has no such function: the semantics are defined here.  gridhip_components_from_image turns every non-zero
 * model cell into a point; this turns a MAP - restored, or any real N x N image, N = gridhip_image_size(theta, lam) - into a
 * catalogue: one row per island of emission with its position, integrated flux and deconvolved shape, in the row format of
 * gridhip_dft_predict, so that the list can be predicted, or solved against, as it is.
 * ISLANDS.  border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac and min_cells are auto-masking's, with the same
 * meaning, the same rounding of the levels T_hi and T_lo, the same rule for the noise pointer (one double; on the device for
 * the _dev and imager forms) and the same reasons 2 and 3.  There is no `absolute`: a catalogue is of positive emission.
 * The islands are the components of K of auto-masking's steps 1-3, before any growing: the components of L = { v > T_lo }
 * that hold a cell of a component of H = { v > T_hi } with at least min_cells cells.  An island's label is its smallest
 * cell index; the islands are listed in ascending label order, so the list is a function of the image alone.  Since the
 * levels are >= 0 every cell of an island is > 0 and all weights below are positive.  An island with several peaks (a
 * blend) is ONE component unless the option "sources_deblend" is set: see DEBLENDING.
 * PER ISLAND, over its cells I(y, x):
 *     exact     ncells; the bounding box y0, y1, x0, x1; the peak P_i and its cell (yp, xp) - the maximum under
 *               image_stats' key order, the smallest cell index among equals; edge = the box touches row or column `border`
 *               or N - 1 - border
 *     sums      with dx = x - xp, dy = y - yp (exact small integers, so that nothing cancels):
 *               S = sum I, Sx = sum I dx, Sy = sum I dy, Sxx = sum I dx^2, Sxy = sum I (dx dy), Syy = sum I dy^2,
 *               each term ONE rounded product of I and an exact integer, added in fp64 in an order that depends on the
 *               island's box and the launch constants only - no floating-point atomics: two runs and all three forms give
 *               the same bits
 *     derived, in this order, every operation rounded (no fused multiply-add):
 *     1  cx = xp + Sx / S, cy = yp + Sy / S; mxx = Sxx / S - (Sx / S)^2, mxy = Sxy / S - (Sx / S)(Sy / S), myy = Syy / S -
 *        (Sy / S)^2; F = S
 *     2  correct != 0: the truncation of a Gaussian cut at an isophote.  t = T_lo / P_i; t == 0 leaves everything as it is;
 *        else F <- F / (1 - t) and m.. <- m.. (1 - t) / (1 - t (1 - ln t)).  (In the coordinates where the Gaussian is
 *        round, P exp(-r^2 / 2) is above t P for r^2 / 2 < -ln t: the flux inside is (1 - t) of the whole and the second
 *        moment inside is 1 - t (1 - ln t) of the whole, so the normalised moment is low by their quotient - for any
 *        axis ratio and angle, for a continuous Gaussian.)
 *     3  beam != NULL (the 8 doubles of gridhip_fit_beam, exp(-(A dx^2 + 2 B dx dy + C dy^2))): det = A C - B^2, the beam's
 *        covariance is bxx = C / (2 det), bxy = -B / (2 det), byy = A / (2 det); F <- F sqrt(det) / pi turns units per beam
 *        into integrated flux; i.. = m.. - b...  Without a beam i.. = m...  A beam that gridhip_restore could not use (ok 0
 *        or NaN, or A, B, C not finite and positive definite) gives NaN in F, bmaj, bmin, bpa of every row and sets flag
 *        bit 2; nothing is silently replaced.  gridhip_find_sources, which has the beam on the host, refuses it instead
 *        (GRIDHIP_EINVAL), as gridhip_restore does.
 *     4  ixx > 0, iyy > 0 and D = ixx iyy - ixy^2 > 0: a Gaussian.  lambda+ = (ixx + iyy) / 2 + sqrt(((ixx - iyy) / 2)^2 +
 *        ixy^2), lambda- = D / lambda+ (the other eigenvalue without its cancellation); FWHM+- = sqrt(8 ln 2 lambda+-)
 *        cells; bmaj, bmin = FWHM+- theta / N; phi = atan2(2 ixy, ixx - iyy) / 2, bpa = pi / 2 - phi folded into (-pi/2,
 *        pi/2]: gridhip_dft_predict's angle, from +m towards +l.  Otherwise a point: bmaj = bmin = bpa = 0, flag bit 0.
 *        This atan2(y, x) is formed from rounded +, -, *, / alone, so that the angle has the same bits wherever it is
 *        computed (a libm's is not correctly rounded): 0 for y = x = 0; t = min(|x|, |y|) / max(|x|, |y|); if t > tan(pi/8)
 *        = 0.4142135623730950488, t <- (t - 1) / (t + 1) and base = pi / 4, else base = 0; s = 1 - z / 3 + z^2 / 5 - ... +
 *        z^22 / 45 with z = t t, by Horner from the last term, each coefficient the quotient 1 / (2 k + 1); r = base + t s;
 *        r <- pi / 2 - r if |y| > |x|; r <- pi - r if x < 0; the sign of y.  Within 1e-15 relative of the true value.
 *     5  l = theta (cx - N/2) / N, m = theta (cy - N/2) / N with the integer N/2, the product before the quotient, as for
 *        gridhip_components_from_image.
 * DEBLENDING.  The option "sources_deblend" = r, 1 <= r <= 32, read when a call is enqueued (0, the default: everything
 * above, bit for bit; above 32: GRIDHIP_EINVAL from all three forms), splits an island into one component per peak.  Islands,
 * levels, min_cells, border and the noise rule are unchanged.  Within an island the cells are ordered by value, and among
 * equal values the smaller cell index ranks higher - image_stats' key order (all values are finite and > 0, so comparing
 * values is comparing keys).
 *     1  up-pointer: for every cell k of K, up[k] is the highest-ranked cell among k and those of its 8 neighbours that lie
 *        in K and carry k's island label.  Neighbours outside the image, outside K or in another island do not count.
 *     2  summits: a cell with up[k] == k looks at the cells of its own island within Chebyshev distance r, the window
 *        clipped at the image; W(k) is the highest-ranked of them, k included.  W(k) != k: up[k] = W(k), the basin climbs on
 *        to a strictly higher cell (which need not be a peak itself).  W(k) == k and image[k] > T_hi: k is a PEAK.  W(k) ==
 *        k and image[k] <= T_hi: k is a faint summit and up[k] is the island's brightest cell, the highest in the order -
 *        always above T_hi and always a peak, so every island keeps at least one row.
 *     3  basins: sub[k] is the fixed point of following up from k; every step goes to a strictly higher cell, so there is
 *        no cycle.  The component of a peak p is { k in K : sub[k] == p }; the components of an island partition its cells.
 *     4  rows: one per peak, in ascending order of the peak's cell index, each measured exactly as an island is, by PER
 *        ISLAND and the steps 1 to 5 over its own cells: ncells, box, peak, the six sums about the peak, `correct` with the
 *        row's own P_i, beam, shape, l and m.  `correct` assumes a cut at an isophote; a basin is cut by a watershed line
 *        where it meets another, and for such a row the correction is approximate.  info[.][0] stays the ISLAND's label, its
 *        smallest cell index, so the rows of one island share it; (yp, xp) is the peak; flag bit 3 (value 8) is set on every
 *        row whose island has more than one row; count, stats[3] and stats[4] count components.  An island with one peak
 *        gives the same comps row and the same info[1:16] bits as with the option off; only the order of the rows can differ.
 *     Only integer comparisons decide anything, so sub is an exact function of the image, and every statement about
 *     determinism in this section holds as it stands: the three forms, two runs and a replayed graph give the same bits.
 * OUTPUTS
 *     comps   [max_c][GRIDHIP_COMP_DOUBLES] rows { l, m, F, 0, 0, 0, bmaj, bmin, bpa, 0 }
 *     info    [max_c][GRIDHIP_SRC_DOUBLES = 16] rows { label, ncells, yp, xp, P_i, S, Sx, Sy, Sxx, Sxy, Syy, y0, y1, x0, x1,
 *             flags }, or NULL.  flags: bit 0 a point, bit 1 edge, bit 2 the beam is unusable, bit 3 one of several rows of
 *             its island (DEBLENDING)
 *     count   one int64 (on the device for the _dev and imager forms): the islands found (with DEBLENDING: the components),
 *             even above max_c.  Only the first max_c rows are written; the rows after the last one written are left as they
 *             were
 *     stats   8 doubles { T_hi, T_lo, P, islands found, rows written, of them points, the sum of F over the rows written
 *             (added in row order by one thread), reason }.  reason 2 and 3 as for auto-masking: count is 0, the counts
 *             are 0 and no row is written
 * Arguments, checked before anything is touched.  GRIDHIP_EINVAL: auto-masking's rules for N, border, image, the levels,
 * noise and min_cells; max_c < 0; a NULL comps with max_c > 0; a NULL count or stats; correct outside {0, 1}; comps, info,
 * count or stats overlapping each other, the image, the beam or the noise.  Then GRIDHIP_EUNSUPPORTED: N > 46340.
 * gridhip_find_sources is synchronous and stages host arrays through the context's pool.  The _dev and imager forms
 * enqueue kernels only on the context's stream - 17 launches whatever the image holds (12 with max_c = 0), no memset or
 * copy node - allocate nothing after the first call of a shape, read nothing back and never synchronise: image ->
 * image_stats -> find_sources -> dft_predict can be captured into one graph.  Scratch is auto-masking's (9 bytes per cell)
 * and 12 B per 1024 cells and 20 B per row; the imager form keeps its own.  With DEBLENDING: 23 launches whatever the image
 * holds (18 with max_c = 0) - 17 and 12 as before with the option at 0 - and 16 B per cell more (the islands' largest value,
 * 8 B, reused for their peak counts; its cell, 4 B; sub, 4 B; up lies in the plane the labelling leaves free), drawn from the
 * context's pool for the length of the call by all three forms, and only when the option is not 0.  A captured graph keeps
 * the address of that pooled block (as it does of the scratch of gridhip_find_sources_dev): replay it on the context's stream
 * only, between calls of the same context and not concurrently with them, and not after the context has met an
 * out-of-memory condition, which frees pooled blocks.
 * The labelling is auto-masking's own kernels.  Then: the roots of the islands are compacted in order (per-segment counts,
 * an exclusive scan, a scatter - components_from_image's pattern), which numbers the rows; one flat pass takes the boxes by
 * 32-bit integer atomicMin / atomicMax per row; one work-group of 256 threads per row walks the row's box in row-major
 * order, thread t the cells t, t + 256, ..., keeping the cells that carry the island's label - first for the peak, then for
 * the count and the six sums - each reduced by a wave shuffle tree and a fixed tree over the four waves; one thread derives
 * the fields and writes both rows.  DEBLENDING is a relabelling in front of that: each island's largest value by a 64-bit
 * integer atomicMax of its bits and then the smallest cell that holds it by a 32-bit atomicMin; up per cell; a wave per summit
 * scans the window; every cell follows up to its fixed point (the cost of a cell is the length of its ascent); and the same
 * compaction, box and measuring kernels run on sub, where a root is a peak. */
#define GRIDHIP_SRC_DOUBLES 16
int gridhip_find_sources(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                         double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                         int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps, double *info,
                         int64_t *count, double *stats);
int gridhip_find_sources_dev(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                             double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                             int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps, double *info,
                             int64_t *count, double *stats);
/* gridhip_find_sources_dev with the imager's theta, lam and N and its own scratch */
int gridhip_imager_find_sources_dev(gridhip_imager *imager, const double *image, int64_t border, double thr_hi, double thr_lo,
                                    double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                                    int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps,
                                    double *info, int64_t *count, double *stats);

/* ---- phase shift and averaging: a stream rotated to another phase centre, groups of samples collapsed into one each ----------
 * The reference has neither: the semantics are defined here.  Every other step runs on the stream at its recorded
 * resolution and about its recorded phase centre; these are the two data-reduction steps a pipeline puts in front of them.
 * PHASE SHIFT.  gridhip_phase_shift rotates n visibilities and their (u, v, w) - wavelengths, un-mirrored, uv_stride as
 *     everywhere else, w == NULL meaning w = 0 - to another phase centre.  R is 9 HOST doubles in both forms, row-major, read
 *     at the call: the rotation from the old (u, v, w) frame to the new one.  Its third row is the new centre (l0, m0, n0) in
 *     the old frame.
 *     PHASE RULE       vis_out = vis_in * exp(+2 pi i p),  p = u l0 + v m0 + w (n0 - 1),
 *                      n0 - 1 = -r2 / (1 + sqrt(1 - r2)), r2 = l0^2 + m0^2 (formed once per call; the subtraction form
 *                      cancels).  The sign, the reduction to turns r = p - rint(p) (exact) and fp64 are exactly those of
 *                      gridhip_dft_predict, with the opposite sign of the exponent: a point of flux S at (l0, m0) therefore
 *                      becomes the constant S.  The product is (re c - im s, re s + im c) with c, s the cosine and sine of
 *                      2 pi r, every product rounded, no fused multiply-add.  With |p| <= 1e4 turns the error of a
 *                      visibility is below 1e-10 |vis|.
 *     COORDINATE RULE  with the coordinate outputs given (all three or none)
 *                          u' = (R00 u + R01 v) + R02 w,  v' = (R10 u + R11 v) + R12 w,  w' = (R20 u + R21 v) + R22 w:
 *                      every product is rounded, the sums go left to right, contraction is off - numpy reproduces them to
 *                      the bit.  They are written at out_stride.
 *     ALIASING         vis_out == vis_in is allowed, and so are u_out == u, v_out == v and w_out == w at out_stride ==
 *                      uv_stride (element k is read before it is written, by the same lane).  Any other overlap of an
 *                      output with an input or with another output is GRIDHIP_EINVAL; the columns of one interleaved (n, 3)
 *                      array do not overlap each other.
 *     NOT FINITE       a visibility with a non-finite u, v or w passes vis_in through unchanged and is counted; its
 *                      coordinate outputs are what the coordinate rule gives (not finite).
 *     stats            optional, 4 doubles { visibilities shifted, visibilities with non-finite coordinates, 0, 0 }.
 *     Refused before anything is touched, GRIDHIP_EINVAL: a NULL context or R; R not finite; R22 <= 0 (a centre behind the
 *     sky); |R R^T - I| above 1e-9 in any entry; n < 0; a NULL u, v, vis_in or vis_out with n > 0; a stride < 1; one or two of
 *     the three coordinate outputs.  n of 2^31 - 256 or more is GRIDHIP_EUNSUPPORTED.  n = 0 is valid.
 * AVERAGING.  gridhip_average collapses the n samples into G, one per group: group is n int64 as gridhip_flag_residuals
 *     takes it (NULL with G == 1: one group); x (n doubles or NULL: 0) is any further per-sample column - gridhip_dft_predict's
 *     fractional frequency, a time; wt the data weights s_k (n doubles, or NULL for all ones).
 *     CLASSES.  Each visibility falls into the FIRST class that applies:
 *         FLAGGED       s_k is not > 0 (zero, negative, NaN) - gridhip_weights' rule
 *         LEFT OUT      g_k outside [0, G)
 *         NOT FINITE    any of s re, s im, s u, s v, s w, s x is not finite: each is one rounded product, judged on the
 *                       value fp64 computes (1e300 with the weight 1e10 counts)
 *         PARTICIPANT   everything else
 *     SUMS.  They are EXACT INTEGER SUMS, so that the result does not depend on the arrival order.  For each group: n_g is
 *         the number of participants and L = ceil(log2 n_g) as an integer (0 for n_g = 1).  For each class of columns -
 *         vis: re and im; uvw: u, v and w; x; the weight - b is the largest biased exponent field (0 .. 2046) of the
 *         class's weighted values over the group's participants, and s = 1084 - L - b.  Every weighted value y enters as
 *             q = (int64) rint(ldexp(y, s)),   so |q| <= 2^(62 - L)
 *         and the group's sum Q cannot overflow int64.  The column's sum is ldexp((double) Q, -s): one rounding in the
 *         conversion (and the rounding of ldexp where that result is subnormal).
 *         ERROR BOUND against the exact sum:  |sum - exact| <= n_g 2^(L-62) M + 2^-53 |sum|,  M = max(max|y|, 2^-1022)
 *         with max|y| over the class - at most n_g roundings of half the quantum 2^-s, which is <= 2^(L-61) max|y| while the
 *         largest value is normal and stays 2^(L-1084) below that; and the conversion, half an ulp of the sum.  For sums of
 *         mixed sign in the normal range this is within (n_g 2^(L-62) + 2^-52) max|y|.  A class of subnormals with n_g <=
 *         1024 is summed exactly.
 *     OUTPUTS per group: wt_out = W, the weight sum; vis_out = sum / W, and u_out, v_out, w_out (at out_stride) and x_out
 *         the same way, each one rounded division; count_out (int64, may be NULL) = n_g.  A group without participants
 *         gives vis = u = v = w = x = 0, wt = +0.0 and count = 0: a sample every other step already ignores.  x_out may be
 *         NULL when x is.
 *     stats  optional, 8 doubles { groups with a participant, participants, flagged, left out, not finite, largest n_g,
 *         non-finite coordinates seen by the fused shift, 0 }.
 *     FUSED SHIFT.  R != NULL is DEFINED BY THE CALLS IT REPLACES,
 *             gridhip_phase_shift_dev(R: vis, u, v, w -> vis', u', v', w')
 *             gridhip_average_dev(NULL: vis', u', v', w')
 *         with the same bits, and no shifted stream is written.  The shift sees all n visibilities: its count of non-finite
 *         coordinates does not depend on the classes.
 *     Refused before anything is touched, GRIDHIP_EINVAL: a NULL context; n < 0; G < 1; with n > 0 a NULL group unless G == 1 and a NULL
 *     u, v or vis; a stride < 1; a NULL u_out, v_out, w_out, vis_out or wt_out; x without x_out; R as above; any
 *     output overlapping an input or another output.  n of 2^31 - 256 or more and G above 2^31 - 256 are
 *     GRIDHIP_EUNSUPPORTED (the counts are 32-bit).  n = 0 is valid: every group is empty.
 * The host forms are synchronous and stage through the context's pool.  The _dev forms take device pointers (R excepted) and
 * enqueue kernels only on the context's stream - no memset node, no copy node (the tables are zeroed by a kernel); they
 * allocate nothing after the first call of a shape (the scratch - 76 B per group: a 32-bit count, four 32-bit exponents,
 * seven 64-bit sums - comes from the context's pool), never synchronise and read nothing back, so they can be captured
 * into a graph.  An averaging is a fixed number of launches whatever the data hold, 5 (4 without stats): a kernel that
 * zeroes the tables; pass A over the stream - the classes, n_g by 32-bit atomicAdd and b by 32-bit atomicMax; pass B over
 * the stream again - the 64-bit integer atomicAdd of every q; a pass over the groups that finalises; the stats.  The fused
 * shift is evaluated in both passes.  The tables are column-major, so a stream whose neighbours lie in neighbouring groups
 * adds to contiguous memory; where neighbours share a group, the lanes of a wave that form a run of one group are summed by
 * shuffles first and one lane goes to memory.
 * DETERMINISM.  integer atomics only: no floating-point atomic and no sum of doubles.  Integer adds commute, so neither the
 * arrival order nor the pre-aggregation changes a bit: the same bits for the host and _dev forms, for two runs, for any
 * permutation of the stream, and for a numpy restatement with Python's exact integers. */
int gridhip_phase_shift(gridhip_ctx *ctx, int64_t n, const double *R, const double *u, const double *v, const double *w,
                        int64_t uv_stride, const double *vis_in, double *vis_out, double *u_out, double *v_out, double *w_out,
                        int64_t out_stride, double *stats);
int gridhip_phase_shift_dev(gridhip_ctx *ctx, int64_t n, const double *R, const double *u, const double *v, const double *w,
                            int64_t uv_stride, const double *vis_in, double *vis_out, double *u_out, double *v_out,
                            double *w_out, int64_t out_stride, double *stats);
int gridhip_average(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                    const double *v, const double *w, int64_t uv_stride, const double *x, const double *vis, const double *wt,
                    double *u_out, double *v_out, double *w_out, int64_t out_stride, double *x_out, double *vis_out,
                    double *wt_out, int64_t *count_out, double *stats);
int gridhip_average_dev(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                        const double *v, const double *w, int64_t uv_stride, const double *x, const double *vis,
                        const double *wt, double *u_out, double *v_out, double *w_out, int64_t out_stride, double *x_out,
                        double *vis_out, double *wt_out, int64_t *count_out, double *stats);

/* ---- reprojection and mosaicking: images on other tangent planes brought onto one plane and combined, on the device --------
 * The reference has neither: the semantics are defined here.  gridhip_phase_shift makes a stream about any centre, so that any
 * patch of the sky - a facet - is imaged about its own centre; gridhip_mosaic brings F such images back onto ONE tangent plane,
 * and gridhip_reproject, its F = 1 case, also takes a model on the full plane to a facet's plane for gridhip_imager_predict_dev.
 *     facets    F contiguous Ns x Ns real fp64 images, row-major [f][y][x], all with the field of view theta_s.  Cell (x, y)
 *               lies at l = theta (x - N/2) / N, m = theta (y - N/2) / N (N/2 the integer half): gridhip_dft_predict's
 *               convention.
 *     weights   NULL, or F x Ns x Ns fp64 laid out the same way: a primary-beam power, an inverse variance.
 *     R         F x 9 doubles, row-major: R_f is the rotation from the DESTINATION frame to facet f's frame - exactly what
 *               gridhip_phase_shift was given to make that facet.  HOST memory in the host form; DEVICE memory in the _dev
 *               form, so that a call can be captured with any F: a prologue kernel of every call judges it on the device.
 *               A facet whose R_f is not finite, has R22 <= 0 or has an entry of |R R^T - I| above 1e-9 (phase_shift's rule)
 *               contributes nothing and is counted: it is not an error.
 *     out       Nd x Nd, field of view theta_d.  wsum (may be NULL): Nd x Nd, the weight sum of every cell.
 *     kind      0 nearest cell, 1 bilinear, 3 Keys' cubic convolution (a = -1/2).
 *     inner, outer   the feather window in facet cells, measured from the facet's centre cell Ns/2 on either axis.
 * THE RULE FOR ONE DESTINATION CELL (x, y).  Every product and sum is rounded, contraction is off, sums go left to right.
 *     1. l = theta_d (x - Nd/2) / Nd, m likewise, r2 = l l + m m.  If not r2 < 1 the cell lies BEYOND THE HORIZON: it is
 *        blank and no facet is looked at.  Otherwise n = sqrt(1 - r2).
 *     2. For f = 0 .. F-1 in ascending order, over the valid facets only:
 *            l' = (R00 l + R01 m) + R02 n,  m' = (R10 l + R11 m) + R12 n,  n' = (R20 l + R21 m) + R22 n.
 *        If not n' > 0 the facet does not cover the cell.
 *     3. fx = (l' * Ns) / theta_s + (double)(Ns/2), fy likewise from m'.
 *     4. WINDOW.  dx = |fx - Ns/2|, dy likewise.  s(d) = 1 if d <= inner; else 0 if d >= outer; else with
 *            t = (outer - d) / (outer - inner),   s(d) = (t t) (3 - 2 t).
 *        w = s(dx) s(dy).  If w == 0 the facet does not cover the cell.
 *     5. SAMPLE v.
 *            kind 0   the cell (floor(0.5 + fx), floor(0.5 + fy)): the gridders' tie rule.
 *            kind 1   i = floor(fx), t = fx - i; a row is a (1 - t) + b t; the two rows are combined the same way in y.
 *            kind 3   taps i-1 .. i+2 with the coefficients in Horner form
 *                         c0 = ((-0.5 t + 1) t - 0.5) t      c1 = ((1.5 t - 2.5) t) t + 1
 *                         c2 = ((-1.5 t + 2) t + 0.5) t      c3 = ((0.5 t - 0.5) t) t
 *                     a row is ((c0 a + c1 b) + c2 c) + c3 d; the four rows are combined the same way in y.
 *        ALL TAPS of the footprint must lie inside the facet, otherwise the facet does not cover the cell (Ns < 4 never
 *        covers anything with kind 3, Ns < 2 nothing with kind 1).  If any tap is not finite the sample is LEFT OUT and
 *        counted.
 *     6. With a weight image: q = its bilinear sample at (fx, fy), which needs the bilinear footprint inside the facet; if
 *        q is not finite or not > 0 the facet does not cover the cell; otherwise w = w q.
 *     7. num = num + w v, den = den + w.  A facet that does not cover a cell CONTRIBUTES NOTHING - not 0 * v: a NaN under a
 *        zero weight or outside the window never reaches the output.
 *     8. Where den > wmin: out = num / den if normalize, else num; wsum = den.  Otherwise out = blank and wsum = +0.0.
 *     stats     optional, 8 doubles { destination cells covered, cells blank, facets used, facets refused, facet samples
 *               left out because a tap was not finite, the largest number of facets covering one cell, 0, 0 }.
 * gridhip_reproject is gridhip_mosaic with F = 1, no weight image, normalize = 1, wmin = 0 and neither wsum nor stats: the
 * same body.  The way back from the full plane to facet f is R_f^T.
 * Refused before anything is touched, GRIDHIP_EINVAL: a NULL context, facets, R or out; F < 1, Ns < 1 or Nd < 1; a theta
 * that is not finite or not > 0; kind outside {0, 1, 3}; inner < 0, outer < inner or either not finite; wmin negative or
 * NaN; any output overlapping an input or another output.  F above 4096 and Ns or Nd above 32768 are GRIDHIP_EUNSUPPORTED.
 * The host forms are synchronous and stage through the context's pool.  The _dev forms take device pointers and enqueue
 * kernels only on the context's stream - no memset node, no copy node; the scratch (256 B and 80 B per facet) comes from the
 * context's pool, so nothing is allocated after the first call of a shape; they never synchronise and read nothing back, so
 * they can be captured into a graph.  A call is 2 launches, 3 with stats: the prologue that judges every R_f; one thread per
 * destination cell in 16 x 16 tiles, each tile first culling the facets into a list in LDS, in ascending order - the
 * accumulation order, so the cull changes no bit (option "mosaic_cull") - by a bound that holds on the sphere: the tile's
 * box in (l, m, n), on which R is linear (mosaic.hip); the stats.
 * DETERMINISM.  every cell's sums belong to one thread: no floating-point atomic, no order that depends on scheduling; the
 * counts use integer atomics.  fp64 multiply, add, divide, sqrt and floor are correctly rounded, so the bits are the same
 * for the host and _dev forms, for every run, and for a numpy restatement of the rule (tests/mosaic_ref.py).
 * OUT OF SCOPE.  flux conservation for Jy-per-pixel models (a pixel's solid angle changes between planes: a component list
 * through gridhip_components_from_image is the exact route); Lanczos or sinc kernels; primary-beam models. */
int gridhip_mosaic(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                   const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank, int64_t Nd,
                   double theta_d, double *out, double *wsum, double *stats);
int gridhip_mosaic_dev(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                       const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank,
                       int64_t Nd, double theta_d, double *out, double *wsum, double *stats);
int gridhip_reproject(gridhip_ctx *ctx, int64_t Ns, double theta_s, const double *image, const double *R, int kind,
                      double inner, double outer, double blank, int64_t Nd, double theta_d, double *out);
int gridhip_reproject_dev(gridhip_ctx *ctx, int64_t Ns, double theta_s, const double *image, const double *R, int kind,
                          double inner, double outer, double blank, int64_t Nd, double theta_d, double *out);

/* ---- w-stacking: layered grids, image-plane w-screens, a stacked prediction -----------------------------------------------
 * The third way to correct the w-term, beside w-projection (w_cache_imaging: one kernel per w-plane of the whole stream,
 * whose support grows with |w| theta^2) and facets (phase_shift, then mosaic).  The w range is cut into layers of M planes
 * of `wstep`; a layer is gridded on its own with w-projection kernels of the RESIDUAL w only, transformed to the image
 * plane, multiplied there by the exact w-screen of the layer's centre, and the layers are summed.  The kernel table has M
 * planes, whatever the stream's w range, and carries at most M wstep / 2 of |w|.  (Citations: oracle/gridref_np.py;
 * tests/wstack_ref.py is the numpy restatement of this section.)
 * INPUTS.  (theta, lam), N = gridhip_image_size(theta, lam); wstep >= 1; M >= 1 planes per layer; the w-kernel shape
 * (qpx, npixFF, npixKern) under the w-kernel shape rule (at gridhip_w_kernel) - or qpx == 0, IMAGE-DOMAIN LAYERS below; a stream u, v, w in wavelengths (uv_stride as
 * everywhere).
 * PLANES AND LAYERS.  p_k = round(w_k / wstep) (libm round, half away from zero: acc_round, the plane of gridhip_wbins);
 * pmin, pmax over the visibilities with a finite w; L = (pmax - pmin) div M + 1 layers; layer_k = (p_k - pmin) div M; the
 * centre plane of layer l is pc_l = pmin + l M + M div 2; the residual bin r_k = p_k - pc_l + M div 2 lies in [0, M).  A
 * visibility with a non-finite w has no layer: it grids nothing and predicts exactly 0 (vis_sub[k] in the residual form),
 * and is counted by gridhip_last_dropped (and by gridhip_wstack_info) together with what the layers' gridder drops.
 * L > 4096, M > 65536, n >= 2^31 - 256 or |p| > 2^52 is GRIDHIP_EUNSUPPORTED.  n = 0 (or no finite w) gives L = 0, a zero
 * image and no error.
 * KERNEL TABLE.  One for all layers: K[r] = conj(w_kernel(theta, (r - M div 2) wstep, npixFF, npixKern, qpx)), r in [0, M).
 * SCREEN.  c_i = (i - N div 2) / N theta; ph[y, x] = 1 - sqrt(1 - c_x^2 - c_y^2); S_l[y, x] = exp(-2 pi i pc_l wstep
 * ph[y, x]), and 0 where c_x^2 + c_y^2 >= 1.  The minus sign is the one that makes S_l conj(far field of K) the far field of
 * conj(w_kernel(w)); with a plus the error against a direct Fourier sum triples (tests/test_wstack_host.py).
 * IMAGE.  G_l = convgrid2(K, 0, u / lam, v / lam, r, vis) over the visibilities of layer l; D = sum_l S_l x ifft_c(G_l);
 * gridhip_wstack_image_dev writes image = Re(D), N x N doubles, overwritten.  An empty layer contributes nothing and costs
 * nothing: no clear, no transform.
 * PREDICT.  The exact adjoint: for k in layer l, pred_k = degrid2(conj(K), fft_c(conj(S_l) x model), u / lam, v / lam, r)_k,
 * written at the visibility's own index; vis_out = pred, or vis_sub - pred; vis_out == vis_sub is allowed.  For any vis
 * and any real model   sum(model * image(vis)) == N^-2 Re(vdot(vis, predict(model))).
 * THE HANDLE.  A gridhip_wstack behaves like a gridhip_plan: it binds the stream as given (no mirror, no weights), owns
 * everything it needs (the layer-ordered coordinates, one gridhip_plan per occupied layer, the two kernel tables, two
 * N x N grids, its transform), its inputs may be freed once creation returns, and it belongs to its context (same
 * device, same stream, not thread-safe; destroy it before the context).  gridhip_wstack_create_dev synchronises: it reads
 * the plane range and the layers' sizes back, as kind 2 reads its w-bins' range.  After creation, image and predict
 * enqueue kernels and hipFFT executions only - no memset or copy node, nothing read back - and allocate nothing after
 * their first call, so a pass can be captured into a graph.  All arguments are checked before anything is touched
 * (GRIDHIP_EINVAL); a refused creation leaves *ws NULL, a refused pass its outputs as they were.  The order of the
 * visibilities inside a layer's slice is the order the partition's atomic adds arrive in, and the gridder adds with
 * floating-point atomics: an image agrees from run to run to rounding, not to the bit; a prediction is bit-reproducible.
 * gridhip_wstack_info: the layers L, how many of them hold a visibility, pmin, and the dropped visibilities (any may be
 * NULL).
 * DO_IMAGING WITH A STACK.  mirror_uvw; doweight on the mirrored u, v, as every kind; ONE stack on the mirrored stream;
 * image = 2 Re D(wt vis1), psf = 2 Re D(wt); both divided by pmax = max(psf).  DIFFERENCE FROM KINDS 0 TO 2: those
 * return Re(ifft_c(make_grid_hermitian(G))), which equals 2 Re(ifft_c(G)) except for what the gridder put on row 0 or
 * column 0 of an even-N grid - make_grid_hermitian leaves those cells without their mirror image, 2 Re doubles them like
 * every other cell.  A stack cannot apply make_grid_hermitian (its layers' mirror images lie in the layers of -w), so it
 * takes 2 Re throughout.  gridhip_predict_wstack is the stack's predict on the stream as given (no mirror), as
 * gridhip_predict.  Both make a stack for the call and destroy it; the host forms are synchronous, the _dev forms take
 * device pointers (pmax stays a host pointer) and synchronise too.  A major-cycle loop does not call them per cycle: an
 * imager of kind 4 ("imagers") binds both streams once and is defined by these two calls.
 * IMAGE-DOMAIN LAYERS.  qpx == 0 in any of the entry points below (and Q == 0 in an imager of kind 4) selects another
 * way to form a layer's grid G_l: image-domain gridding (van der Tol, Veenboer & Offringa 2018).  npixKern is then the
 * subgrid size Sg, one of 16, 24, 32, and npixFF the margin K, even, 4 <= K <= Sg / 2; anything else is GRIDHIP_EINVAL,
 * checked with the other arguments before anything is touched.  Planes, layers, pmin, L, pc_l, the screens S_l, D = sum_l S_l
 * x ifft_c(G_l), a non-finite w, 2 Re in do_imaging and the limits are as above; the residual bin r is not used and there
 * is no kernel table.  e(p) = exp(2 pi i p); a phase p in turns is reduced, r = p - rint(p), and evaluated by
 * sincospi(2 r).  (tests/idg_ref.py is the numpy restatement of this paragraph.)
 *   Cells and tiles.  T = Sg - K.  x_k = N (u_k / lam) + N div 2 (the product rounded, then the sum), y_k likewise.  A
 *   visibility outside 0 <= x < N, 0 <= y < N (NaN included) is dropped: it grids nothing, predicts exactly 0 (vis_sub[k]
 *   in the residual form) and is counted with the visibilities without a finite w.  Tile tx = floor(x / T), ty likewise;
 *   subgrid origin ox = tx T - K / 2, centre cell cx = ox + Sg / 2; a_k = x_k - cx in [-T / 2, T / 2), b_k likewise;
 *   dw_k = w_k - pc_l wstep, the exact residual w.
 *   Subgrid image.  f_i = (i - Sg / 2) / Sg, l_i = f_i theta, ph[j][i] = 1 - sqrt(1 - l_i^2 - l_j^2);
 *   P[j][i] = sum_k vis_k e(a_k f_i + b_k f_j - dw_k ph[j][i]) over the visibilities of the tile, and 0 where
 *   l_i^2 + l_j^2 >= 1.
 *   Taper.  beta = 1.15 K, t(f) = exp(beta (sqrt(1 - 4 f^2) - 1)), Pt = P t(f_i) t(f_j).
 *   To the grid.  Gs[q][p] = Sg^-2 sum_{j,i} Pt[j][i] e(-((p - Sg / 2) f_i + (q - Sg / 2) f_j)), added to G_l at cell
 *   (oy + q, ox + p); cells outside the grid are skipped, not wrapped, and the visibility is kept.
 *   Correction and trusted region.  c(x) = 1 / t((x - N div 2) / N) where 8 |x - N div 2| <= 3 N, else 0; C[y][x] = c(y)
 *   c(x); image = Re(C x D).  Outside the inner three quarters the image and the PSF are exactly 0, so pmax and every CLEAN
 *   peak search see only cells the taper can be divided out of (C reaches 2.6e5 in the corner at K = 16).
 *   Predict, the exact adjoint.  F_l = fft_c(conj(S_l) x C x model) (the model is read inside the trusted region only); the
 *   Sg x Sg patch of F_l at (oy, ox), 0 outside the grid; p[j][i] = t(f_i) t(f_j) Sg^-2 sum_{q,p'} patch[q][p'] e(+((p' - Sg
 *   / 2) f_i + (q - Sg / 2) f_j)), 0 where l_i^2 + l_j^2 >= 1; pred_k = sum_{j,i} p[j][i] e(-(a_k f_i + b_k f_j - dw_k
 *   ph[j][i])), j outer and i inner in one thread: a prediction is bit-reproducible from run to run, an image agrees to
 *   rounding (the subgrids are added with floating-point atomics).  The adjoint identity above holds.
 *   The handle binds a partition by (layer, tile) - a, b, dw and the stream index of every kept visibility - and a list of
 *   work items, one per occupied tile of a layer, a tile of more than "idg_split" visibilities cut into several (the map is
 *   linear); no gridhip_plan and no table.  The gridder stages a work item's visibilities through LDS "idg_chunk" at a time
 *   (both read-only options).  L x ceil(N / T)^2 above 2^26 is GRIDHIP_EUNSUPPORTED.  Accuracy against a direct Fourier
 *   sum, and cost against the w-projection layers: DESIGN.md, section 9.
 *   An imager of kind 4 with Q == 0: 0 <= x < N is not symmetric under the mirror (x = 0 against x = N; an odd N), so
 *   its two stacks may keep different visibilities; it then takes the stream-order middle pass in every cycle, whatever
 *   "wstack_middle" says, and vis_res and the image are still those of the two calls it replaces. */
typedef struct gridhip_wstack gridhip_wstack;
int gridhip_wstack_create_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                              double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                              int64_t uv_stride, gridhip_wstack **ws);
int gridhip_wstack_image_dev(gridhip_wstack *ws, const double *vis, double *image);
int gridhip_wstack_predict_dev(gridhip_wstack *ws, const double *model, const double *vis_sub, double *vis_out);
int gridhip_wstack_info(gridhip_wstack *ws, int64_t *layers, int64_t *occupied, int64_t *pmin, int64_t *dropped);
int gridhip_wstack_destroy(gridhip_wstack *ws);
int gridhip_do_imaging_wstack(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                              double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                              int64_t uv_stride, const double *vis, double *image, double *psf, double *pmax);
int gridhip_do_imaging_wstack_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                                  double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                                  int64_t uv_stride, const double *vis, double *image, double *psf, double *pmax);
int gridhip_predict_wstack(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                           double theta, int64_t lam, const double *model, int64_t n, const double *u, const double *v,
                           const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out);
int gridhip_predict_wstack_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                               double theta, int64_t lam, const double *model, int64_t n, const double *u, const double *v,
                               const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out);

/* ---- joint deconvolution: P images of one sky cleaned together, on the device --------------------------------------------
 * Several images of the same sky - the Stokes planes of one stream, the channels of a cube - cleaned one by one put their
 * components at different cells and chase each plane's own noise peaks.  Here the search runs on ONE combined statistic and
 * every component is taken at one cell in all planes, each plane with its own peak value and PSF.  The reference has none
 * of this: the semantics are defined here.  All images are real N x N, laid out as gridhip_clean's, c = N / 2.
 *     P in 1 .. 8 planes;  residuals[P][N][N] is updated in place;  models[P][N][N] is accumulated into, never zeroed
 *     psfs[Q][N][N], Q in {1, P}: Q == 1 is one PSF for all planes (Stokes planes of one stream), Q == P a PSF per plane
 *         (channels); plane p uses psfs[Q == P ? p : 0]
 *     weights: a HOST array of P doubles for every form, read at call time as gridhip_msclean's scales are; NULL: all 1.0.
 *         Each is finite and >= 0 and at least one is > 0.  A plane of weight 0 does not steer the search and is still
 *         cleaned at every position found: {1, 0, 0, 0} cleans Q, U, V where I peaks.
 *     metric 0 ("sum"):    s = w_0 * R_0 + w_1 * R_1 + ...
 *     metric 1 ("sumsq"):  s = w_0 * (R_0 * R_0) + w_1 * (R_1 * R_1) + ...
 *         p ascending from the first term, every product rounded, then added; no fused multiply-add
 *     mask, nsigma, noise (ONE double, sigma, where the images are), peak_frac: as for gridhip_clean_auto
 * With d = metric + 1 (x^1 = x, x^2 = x * x rounded once):
 *     first pick: s1 = s at the first peak (NaN when nothing can be selected)
 *         L = max(threshold^d, (nsigma * sigma)^d, (peak_frac^d) * |s1|)      every product rounded once; a term whose
 *             factor is 0 is left out (noise is then not read), and s1's term when s1 does not exist; nsigma > 0 with a
 *             NaN sigma: the call stops at once and touches nothing but stats (reason 3)
 *     repeat at most niter times:
 *         k = the flat index of the largest |s| over border <= y, x < N - border with mask[k] != 0; ties go to the lowest
 *             flat index; a NaN s is never selected (so a NaN in any plane, under any weight, excludes the cell)
 *         nothing selectable: stop, reason 2
 *         |s[k]| <= L: stop, reason 1                 (before anything is subtracted and before the niter test)
 *         for every p:  f_p = gain * R_p[k] (rounded once);  models[p][k] += f_p;  flux_p += f_p   (one fused multiply-add
 *                       each, as gridhip_clean's);  R_p -= f_p * psf_q(p) over gridhip_clean's update region and patch
 *                       rule, the product rounded, then subtracted
 *     stats (GRIDHIP_JCLEAN_STATS = 16 doubles) = { iterations, s at the final k*, k*, L, reason, s1, 0, 0,
 *                       flux_0 .. flux_7 }, k* the peak of the final residuals under the same rule (NaN at -1 when none);
 *                       reason 0: niter components taken; unused flux slots are 0
 * The sumsq stop level is therefore in image units: the polarised intensity sqrt(Q^2 + U^2 + ...) <= T is tested as
 * s <= T * T; no square root is taken anywhere.  No atomics: a call is deterministic bit for bit, and the host and _dev
 * forms give the same bits.  IDENTITY: with P = 1, metric 0 and weights NULL, residuals, models and iterations, final
 * peak, index, flux, T, reason and first peak have the bits of gridhip_clean_auto for the same mask, nsigma, noise and
 * peak_frac.
 * Arguments, checked before anything is touched: gridhip_clean_auto's rules for N, gain, threshold, niter, border, patch,
 * nsigma, peak_frac, noise, NULL pointers and the limit on N; GRIDHIP_EINVAL for P outside 1 .. 8, Q not in {1, P}, a
 * metric other than 0 or 1, a bad weight, or any overlap among the Q + 2P planes and the mask.
 * The shape is gridhip_mfclean's: tiles of 16 x 128 cells and a table of one (score, index) entry per tile; an iteration
 * is a tile kernel over the overlapped tiles - it reads P residuals and Q PSFs and writes P residuals, (2P + Q) * 8 B
 * per cell - and a one-work-group kernel that reduces the table, tests the stop rule and reads the P cells at k.
 * gridhip_jclean is synchronous and stages host arrays through the context's pool.  The _dev form enqueues kernels only
 * on the context's stream (2 + 2 * niter launches; no memset or copy node), allocates nothing after the first call of a
 * shape, never synchronises and reads nothing back: it can be captured into a graph.  Scratch (256 B + 16 B per tile)
 * comes from the context's pool; the state block stops later launches at their first instruction. */
#define GRIDHIP_JCLEAN_STATS 16
int gridhip_jclean(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals, double *models,
                   const double *weights, int metric, double gain, double threshold, int64_t niter, int64_t border,
                   int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac, double *stats);
int gridhip_jclean_dev(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals,
                       double *models, const double *weights, int metric, double gain, double threshold, int64_t niter,
                       int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                       double peak_frac, double *stats);

/* ---- multi-GPU: visibility-sharded gridding + one RCCL fp64 sum all-reduce of the partial grids ------
 * Gridding is linear in the visibility set, so the path shards by visibility with no data-path exchange; the
 * partial N x N grids are summed with ncclAllReduce(ncclDouble, ncclSum) over xGMI.  The
 * reference has no counterpart (single device: app/Main.hs:46-53 picks one (run, runN) pair); these entry points
 * are what its `aw_gridding` / `do_imaging` callers (src/ImageDataset.hs:72-77, src/Gridding.hs:538-541) would
 * bind to use a whole node.  RCCL (librccl.so.1) is loaded on first use.
 *   gridhip_comm_create       ONE process drives ndev devices (ncclCommInitAll); dev_ids NULL = 0..ndev-1.
 *                             The communicator owns one context per device (gridhip_comm_ctx).
 *   gridhip_comm_create_rank  one process per GPU (ncclCommInitRank): rank 0 obtains a 128-byte id with
 *                             gridhip_comm_unique_id and hands it to the other ranks by its own means;
 *                             `ctx` stays the caller's.
 * Failures are described by gridhip_comm_last_error (NULL: the last failure before a communicator existed). */
typedef struct gridhip_comm gridhip_comm;
int gridhip_comm_create(int ndev, const int *dev_ids, gridhip_comm **comm);
int gridhip_comm_unique_id(void *id128);
int gridhip_comm_create_rank(gridhip_ctx *ctx, int nranks, int rank, const void *id128, gridhip_comm **comm);
int gridhip_comm_destroy(gridhip_comm *comm);
const char *gridhip_comm_last_error(const gridhip_comm *comm);
int gridhip_comm_ndev(const gridhip_comm *comm);   /* devices driven by this process */
int gridhip_comm_nranks(const gridhip_comm *comm); /* devices in the communicator */
gridhip_ctx *gridhip_comm_ctx(gridhip_comm *comm, int i);
/* In-place sum over all devices of the communicator of grids[i] (device pointer on this process's i-th device,
 * `cells` complex cells each); enqueued on each context's stream, asynchronous to the host. */
int gridhip_comm_allreduce_grids(gridhip_comm *comm, int64_t cells, double *const *grids);
int gridhip_comm_allreduce_grid(gridhip_comm *comm, int64_t cells, double *grid); /* rank form */
/* The same for rows [y0, y1) of grids of Wd columns only.  A stream that went through mirror_uvw (src/Gridding.hs:551-562:
 * v >= 0) leaves every row below H/2 - gh/2 - 1 of every partial grid exactly zero; reducing from that row on halves the
 * bytes that cross xGMI.  (Rows outside the range keep each device's own partial content.) */
int gridhip_comm_allreduce_rows(gridhip_comm *comm, int64_t Wd, int64_t y0, int64_t y1, double *const *grids);
int gridhip_comm_allreduce_grid_rows(gridhip_comm *comm, int64_t Wd, int64_t y0, int64_t y1, double *grid); /* rank form */
/* Communicator options:
 *   "collective"  0 (default) = one ncclAllReduce; 1 = ncclReduceScatter + ncclAllGather, both in place (rank r owns
 *                 the r-th of nranks equal chunks; the remainder goes through a small all-reduce): the direct schedule
 *                 on xGMI's point-to-point links - every GPU exchanges one chunk with each peer at once */
int gridhip_comm_set_option(gridhip_comm *comm, const char *key, int64_t value);
int gridhip_comm_get_option(gridhip_comm *comm, const char *key, int64_t *value);
/* The hipStream_t device i's collectives are enqueued on.  Default: the context's own stream, i.e. ordered after its
 * gridding calls and before the next one.  A host that wants step i's all-reduce to run beside step i+1's gridding
 * passes a side stream here and orders the two itself (an event recorded after the gridding, waited for by the side
 * stream; python/gridhip/distributed.py: OverlappedCommReducer).  A collective's kernel that becomes ready at the
 * boundary between two steps takes its CUs as the tile kernel's work-groups retire; one that becomes ready in the middle
 * of a persistent tile kernel (the all-gather after the reduce-scatter) waits for its end unless the context options
 * "yield_cus" or "reserve_cus" make CUs come free.
 * gridhip_comm_convgrid2 (synchronous) always reduces on the gridding streams. */
int gridhip_comm_set_stream(gridhip_comm *comm, int i, void *hip_stream);
int gridhip_comm_reset_stream(gridhip_comm *comm, int i);
/* convgrid2 over the communicator, host pointers, synchronous (the drop-in form).  Single-process form: the n
 * visibilities are cut into contiguous shards, one per device, gridded concurrently, the partial grids all-reduced
 * and `grid` (accumulated into) returned.  Rank form: every process passes its own shard; the incoming grid is
 * summed over ranks too, so it should be non-zero on one rank only.
 * Failures: a device whose shard fails locally still takes part in the all-reduce (the other devices / ranks would
 * wait in it for ever otherwise) and the call then returns that device's error with `grid` untouched; the internal
 * consistency counter ("errors") of every local device is checked before the grid is handed back.  In the rank form
 * both are LOCAL verdicts: the other ranks have summed this rank's incomplete grid and return GRIDHIP_OK, so the host
 * must agree on the outcome across ranks before it uses the result. */
int gridhip_comm_convgrid2(gridhip_comm *comm, int64_t H, int64_t Wd, double *grid, int64_t n, int64_t W,
                           int64_t Q, int64_t gh, int64_t gw, const double *gcf, const double *u,
                           const double *v, int64_t uv_stride, const int64_t *wbin, const double *vis);

/* ---- device memory helpers (so a non-HIP host language can stage buffers) ----------------- */
int gridhip_malloc(gridhip_ctx *ctx, void **dptr, int64_t bytes);
int gridhip_free(gridhip_ctx *ctx, void *dptr);
int gridhip_memcpy_h2d(gridhip_ctx *ctx, void *dst, const void *src, int64_t bytes);
int gridhip_memcpy_d2h(gridhip_ctx *ctx, void *dst, const void *src, int64_t bytes);
int gridhip_memset(gridhip_ctx *ctx, void *dptr, int value, int64_t bytes);

/* ---- timing of the last device call (HIP events on the context's stream) ------------------
 * ms_total covers binning pre-pass + tile kernel; ms_kernel the dominant kernel only.
 * Synchronises on the recorded events. */
int gridhip_last_timing(gridhip_ctx *ctx, double *ms_total, double *ms_prepass,
                        double *ms_kernel);
/* the same for the timed call `back` calls before the last one (0 = the last; the last 64 are kept), so that a
 * benchmark loop can collect every step's device times after the loop instead of synchronising inside it */
int gridhip_timing(gridhip_ctx *ctx, int back, double *ms_total, double *ms_prepass, double *ms_kernel);
int gridhip_enable_timing(gridhip_ctx *ctx, int enable);

#ifdef __cplusplus
}
#endif
#endif /* GRIDHIP_H */
