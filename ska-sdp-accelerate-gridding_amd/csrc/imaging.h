// libgridhip internal declarations of the layer around the gridder: the host-pointer forms' staging, the transform, the
// streaming image operations, the imaging functions, prediction, imagers, deconvolution and the restore (api.hip, comm.hip,
// awgrid.hip's entry points, ctx.hip's pool, fft.hip, image_ops.hip, imaging.hip, predict.hip, imager.hip, clean.hip,
// msclean.hip, mfclean.hip, jclean.hip, noise.hip, automask.hip, restore.hip, weights.hip, gaincal.hip, ddcal.hip, dft.hip, flag.hip,
// sumthreshold.hip, sources.hip, average.hip, jonescal.hip, mosaic.hip, wstack.hip, rm.hip, noisemap.hip).  The byte-range rules of the argument checks are in argrules.h, which this file includes.
// The pre-pass and the tile kernels (bin.hip, tile_*.hip, tile_common.h, simple.hip) see none of this: what they are
// compiled from is common.h alone, so that a change here leaves their source fingerprint (bench.py) as it is.
#pragma once
#include <math.h>

#include <utility>
#include <vector>

#include "argrules.h"
#include "common.h"

namespace gridhip {

// The part of a context that belongs to this layer (gridhip_ctx::img; made and freed with the context, ctx.hip).
struct ImagingState {
    // cached hipFFT Z2Z plans (fft.hip): do_imaging with w_cache_imaging alternates between the kernel generator's
    // size and the image's, and creating a plan costs milliseconds
    void *fft_plan[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t fft_n[4] = {0, 0, 0, 0};
    int fft_next = 0;  // the slot the next new size replaces
    // device blocks of the host-pointer forms and the imaging entry points (DevBuf), kept between calls: a repeated
    // call then neither allocates nor frees - hipFree synchronises the whole device.  All of a context's work is
    // ordered on one stream (gridhip_set_stream orders a new one after the old), so a block handed back by one call
    // may be handed out to the next without waiting.
    std::vector<std::pair<void *, size_t>> pool_free;
    // the last w-kernel table w_cache_imaging built (imaging.hip): the table depends on the field of view, the w-planes
    // and the kernel's shape only, and an imaging run calls with the same ones again and again (image and PSF, every
    // major cycle) - a call whose planes match takes the table as it is (21 planes: 1.6 ms of small kernels saved)
    struct {
        double theta = 0.0;
        int64_t wstep = 0, wmin = 0, nplanes = 0, npixFF = 0, S = 0, Q = 0;
        void *ptr = nullptr;
        size_t bytes = 0;
    } wk_cache;
    bool restore_lds_raised = false;  // restore_kernel has been allowed its dynamic LDS on this device (restore.hip)
    bool msconv_lds_raised = false;   // and ms_conv_kernel its own (msclean.hip)
    bool flag_lds_raised = false;     // and flag_hist_kernel's LDS path its 64 KB (flag.hip)
    unsigned int gain_lds_raised = 0;  // and ddcal_iter_kernel<D> its DD_LDS_BUDGET (bit D), jones_iter_kernel its 80 KB (bit 0)
    int64_t noise_bits = 0;           // option "noise_bits": the digit of image_stats' radix select, 8 or (else) 13 bits
    int64_t dft_slices = 0;           // option "dft_slices": the component slices of dft_predict, 0 = by (n, C), 1..64 forced
    int64_t sources_deblend = 0;      // option "sources_deblend": find_sources splits islands at window radius 1..32, 0 = not
    int64_t mosaic_cull = 0;          // option "mosaic_cull": 1 = every tile of gridhip_mosaic walks all valid facets (the same bits)
    int64_t rm_stage = 0;             // option "rm_stage": 1 = gridhip_rmclean reads and writes the cube through LDS (the same bits)
    int64_t noisemap_hist = 0;        // option "noisemap_hist": how noise_map's node kernel builds a histogram (noisemap.hip)
    int64_t wstack_middle = 0;        // option "wstack_middle": 1 = a stack imager's cycle takes the other middle pass (imager.hip)
    bool noisemap_lds_raised = false;// nm_node_kernel has been allowed its 146 KB of dynamic LDS (noisemap.hip)
    int64_t scratch_fill = 0;         // option "scratch_fill" (TEST HOOK): 1..255 = the byte every block is filled with first
    int64_t scratch_filled = 0;       // read-only "scratch_filled": the blocks filled so far (scratch_prefill, ctx.hip)
};

// TEST HOOK (option "scratch_fill"): a block the library is about to use - a pooled one handed out, a workspace that
// grew, a handle's own - is filled with the option's byte, in stream order before whatever the call enqueues next.  Off
// (0): one comparison.  A memset node: not for captured calls.
int scratch_prefill(gridhip_ctx *ctx, void *p, size_t bytes);

// Device block of one call, drawn from and returned to the context's pool (ImagingState::pool_free): the smallest pooled
// block of at least the size asked for and at most twice it, else a new one.  Nothing is freed before gridhip_destroy,
// so the second call of a given shape allocates nothing.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    gridhip_ctx *owner = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;  // (one owner hands the block back)
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (p && owner) owner->img->pool_free.emplace_back(p, cap);
    }
    int alloc(gridhip_ctx *ctx, size_t bytes);
    int upload(gridhip_ctx *ctx, const void *host, size_t bytes);  // alloc, then an async copy of `bytes` from the host
    template <typename T>
    T *as()
    {
        return reinterpret_cast<T *>(p);
    }
};

// copies on ctx->stream (none for 0 bytes); copy_in / copy_out take host arrays (the drop-in forms) or device-resident
// ones (dev: the _dev forms)
static inline int copy_in(gridhip_ctx *ctx, void *d, const void *src, size_t bytes, bool dev)
{
    if (bytes) GH_CHECK_HIP(ctx, hipMemcpyAsync(d, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return GRIDHIP_OK;
}
static inline int copy_out(gridhip_ctx *ctx, void *dst, const void *d, size_t bytes, bool dev)
{
    if (bytes) GH_CHECK_HIP(ctx, hipMemcpyAsync(dst, d, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    return GRIDHIP_OK;
}
static inline int h2d(gridhip_ctx *ctx, void *d, const void *h, size_t bytes) { return copy_in(ctx, d, h, bytes, false); }
static inline int d2h(gridhip_ctx *ctx, void *h, const void *d, size_t bytes) { return copy_out(ctx, h, d, bytes, false); }
static inline int sync(gridhip_ctx *ctx)
{
    GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GRIDHIP_OK;
}

// the host forms' strided coordinate outputs: n contiguous doubles from the device into out[k * stride]; synchronises
// unless stride == 1
int download_strided(gridhip_ctx *ctx, double *out, int64_t stride, const void *dev, int64_t n);

// The pointer arguments of one call as its kernels see them, for both forms of an entry point from one body.  dev: the
// caller's pointers are device pointers and pass through as they are; nothing is allocated, copied or waited for.  Else
// every non-null pointer gets a pooled block (in the order of the calls), inputs are uploaded at once and finish()
// downloads the outputs in that order and synchronises the stream once.  A null pointer stays null either way, also
// where its length is 0 (a null required argument of an empty call gets no block, as in the _dev form).  A block
// that cannot be had makes every later call return null and status() / finish() return its code: a body checks status()
// once, after its last argument and before it launches anything.  Every host-pointer form goes through it - the
// gridders' (api.hip, awgrid.hip: stage, then the _dev form) as the imaging layer's (one X_any body per pair) - but
// gridhip_comm_convgrid2, whose blocks per device outlive the call that stages them (comm.hip).
class Staged {
  public:
    Staged(gridhip_ctx *ctx, bool dev) : ctx_(ctx), dev_(dev) {}
    template <typename T>
    const T *in(const T *p, size_t bytes) { return static_cast<const T *>(block(p, p, nullptr, bytes)); }
    template <typename T>
    T *out(T *p, size_t bytes) { return static_cast<T *>(block(p, nullptr, p, bytes)); }
    // uploaded from src, downloaded to dst (dev: dst itself - a kernel that reads src is given src by the body)
    template <typename T>
    T *inout(const T *src, T *dst, size_t bytes) { return static_cast<T *>(block(dst, src, dst, bytes)); }
    // a block that finish() leaves alone: the body downloads what it wants of it itself
    template <typename T>
    T *raw(T *p, size_t bytes) { return static_cast<T *>(block(p, nullptr, nullptr, bytes)); }
    int status() const { return err_; }
    int finish();

  private:
    void *block(const void *own, const void *src, void *dst, size_t bytes);
    struct Out {
        void *host;
        const void *d;
        size_t bytes;
    };
    static constexpr int MAX = 16;  // pointer arguments of one call (gridhip_average has 15)
    gridhip_ctx *ctx_;
    bool dev_;
    int err_ = GRIDHIP_OK;
    int nbufs_ = 0, nouts_ = 0;
    DevBuf bufs_[MAX];
    Out outs_[MAX];
};

// findClosest, src/Gridding.hs:895-907 (hi clamped to len-1 as the host twin does, ImageDataset.hs:150-168)
__device__ __forceinline__ int64_t closest_index(int64_t nws, const double *__restrict__ ws, double x)
{
    int64_t lo = 0, hi = nws;
    while ((hi - lo) / 2 >= 1) {
        const int64_t mid = (hi + lo) / 2;
        if (x > ws[mid])
            lo = mid;
        else
            hi = mid;
    }
    const int64_t hc = hi > nws - 1 ? nws - 1 : hi;
    return fabs(x - ws[lo]) < fabs(x - ws[hc]) ? lo : hc;
}

// doweight's cell, src/Gridding.hs:564-583: frac_coords (N,N) 1 p; -1: outside the grid or NaN (the weight stays 1)
__device__ __forceinline__ int64_t weight_cell(int64_t N, double pu, double pv)
{
    int64_t x, y;
    int32_t f;
    frac_coord_dev(N, 1, pu, &x, &f);
    frac_coord_dev(N, 1, pv, &y, &f);
    if (!(pu == pu) || !(pv == pv) || x < 0 || y < 0 || x >= N || y >= N) return -1;
    return y * N + x;
}

// A double maximum is kept on the device in ordered-bits form: an order-preserving map of doubles onto unsigned
// integers, so that atomicMax works (real_max_kernel writes it, divide_kernel and the host read it back).
__host__ __device__ constexpr unsigned long long ordered_bits(double x)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    return (b & 0x8000000000000000ULL) ? ~b : (b | 0x8000000000000000ULL);
}
__host__ __device__ constexpr double ordered_value(unsigned long long b)
{
    return __builtin_bit_cast(double, (b & 0x8000000000000000ULL) ? (b & 0x7fffffffffffffffULL) : ~b);
}

// work-groups of 256 threads for a grid-stride loop over n items (at most 16 per CU)
static inline dim3 grid_for(gridhip_ctx *ctx, int64_t n, int block = 256)
{
    int64_t b = (n + block - 1) / block;
    if (b < 1) b = 1;
    if (b > (int64_t)ctx->num_cu * 16) b = (int64_t)ctx->num_cu * 16;
    return dim3((unsigned)b);
}

// ---- the transform (fft.hip): hipFFT is loaded on first use and named nowhere else --------------------------------------
// the context's cached N x N Z2Z hipFFT plan, bound to its stream; an in-place transform with it
int fft_plan_for(gridhip_ctx *ctx, int64_t N, void **out_plan);
int fft_exec(gridhip_ctx *ctx, void *plan, double2 *data, bool inverse);
// a transform the caller owns (hipfftPlan2d Z2Z, N x N), binding it to the context's stream, releasing it
int fft_plan_own(gridhip_ctx *ctx, int64_t N, void **out_plan);
int fft_plan_bind(gridhip_ctx *ctx, void *plan);
void fft_plan_drop(void *plan);
void fft_release(gridhip_ctx *ctx);
// out = the centred transform of in (N x N complex; in is preserved, tmp is scratch, out may not alias in)
int dev_fft2c(gridhip_ctx *ctx, int64_t N, const double2 *in, double2 *out, double2 *tmp, bool inverse);

// ---- streaming operations (image_ops.hip) ------------------------------------------------------------------------------
// out[k] = x[k * stride] / lam (scale_kernel: div3, src/Gridding.hs:838-839)
int launch_scale(gridhip_ctx *ctx, int64_t n, const double *x, int64_t stride, double lam, double *out);
// pu, pv = fresh blocks of u / lam, v / lam (n doubles each)
int scaled_uv(gridhip_ctx *ctx, int64_t n, const double *u, const double *v, int64_t stride, double lam, DevBuf &pu,
              DevBuf &pv);
// du, dv, dw = fresh blocks of the strided columns made contiguous; w may be null (dw is then left unwritten)
int slice_uvw(gridhip_ctx *ctx, int64_t n, const double *u, const double *v, const double *w, int64_t stride, DevBuf &du,
              DevBuf &dv, DevBuf &dw);
// out[y][x] = in[(y+s) mod N][(x+s) mod N] * scale (roll_kernel)
int launch_roll(gridhip_ctx *ctx, int64_t N, const double2 *in, double2 *out, int64_t s, double scale);
// x[c] /= the maximum kept in maxbits in ordered-bits form (divide_kernel)
int launch_divide(gridhip_ctx *ctx, int64_t cells, double *x, const unsigned long long *maxbits);
// mirror_uvw in place (w, vis may be null); doweight: vis[k] /= the number of visibilities in its cell (cnt: N x N
// zeroed counters)
int launch_mirror(gridhip_ctx *ctx, int64_t n, double *u, double *v, double *w, double2 *vis);
int launch_doweight(gridhip_ctx *ctx, int64_t N, int64_t n, const double *pu, const double *pv, unsigned int *cnt,
                    double2 *vis);
// the imaging tail: out = real(ifft_c(make_grid_hermitian(g))), its maximum into *maxbits when given, or (divbits)
// stored divided by the maximum kept there; h: N x N complex scratch; plan: fft_plan_own's, or the context's
int image_tail(gridhip_ctx *ctx, int64_t N, const double2 *g, double2 *h, double *out, unsigned long long *maxbits,
               const unsigned long long *divbits = nullptr, void *plan = nullptr);
// image and psf divided by the PSF's maximum that maxbits holds (image_tail's); *pmax gets it.  Synchronises.
int normalise(gridhip_ctx *ctx, size_t cells, double *image, double *psf, const unsigned long long *maxbits, double *pmax);
// the w-bin rule on the device (synchronises: min and plane count come back to the host)
int dev_wbins(gridhip_ctx *ctx, int64_t n, const double *w, int64_t stride, int64_t wstep, int64_t *wbin, int64_t *wmin,
              int64_t *nplanes);
// The w-kernel shape rule (include/gridhip.h, at gridhip_w_kernel): wkern_extract_kernel reads the na x na transform from
// row and column na / 2 - Q * (S / 2) - (Q - 1) to na / 2 - Q * (S / 2) + Q * (S - 1); the first is negative unless
// na / 2 - Q * (S / 2) >= Q - 1, the last is below na for S <= npixFF.  Every caller-given shape passes through here.
static inline bool w_kernel_shape_ok(int64_t npixFF, int64_t S, int64_t Q)
{
    return npixFF > 0 && S > 0 && Q > 0 && S <= npixFF && (npixFF * Q) / 2 - Q * (S / 2) >= Q - 1;
}
// one plane of a w-kernel table, out[Q][Q][S][S]; pad: (npixFF * Q)^2 complex scratch
int dev_w_kernel(gridhip_ctx *ctx, double theta, double w, int64_t npixFF, int64_t S, int64_t Q, double2 *out, bool conj,
                 double2 *pad);
// table[nplanes][Q][Q][S][S]: the w-kernels of the planes w = i * wstep + wmin (src/Gridding.hs:434-448), conjugated or not
int build_w_planes(gridhip_ctx *ctx, double theta, int64_t wstep, int64_t wmin, int64_t nplanes, int64_t npixFF, int64_t S,
                   int64_t Q, double2 *table, bool conj);

// ---- pieces of predict.hip that imager.hip shares -----------------------------------------------------------------------
// f = fft_c(model) (N x N complex); t: N x N complex scratch, used for odd N only; plan as image_tail's
int model_transform_to(gridhip_ctx *ctx, int64_t N, const double *model, double2 *f, double2 *t, void *plan);
int launch_simple_degrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double2 *grid, int64_t n, const double *u,
                         const double *v, int64_t stride, double lam, double2 *out);
int launch_conj_copy(gridhip_ctx *ctx, int64_t n, const double2 *in, double2 *out);
int launch_residual(gridhip_ctx *ctx, int64_t n, const double2 *pred, const double2 *sub, double2 *out);
// A plan that an imager gathers with: the caller clears the predictions itself (in a kernel, so that a cycle can be
// captured) where the plan would clear them with a memset.  Returns whether they need clearing at all.
bool plan_caller_clears(gridhip_plan *plan);
bool aw_plan_caller_clears(gridhip_aw_plan *plan);

// ---- the imaging functions (imaging.hip) --------------------------------------------------------------------------------
// Which ImagingFunction (src/Gridding.hs:76-81) a call images or predicts with, and its options:
//   kind 0 simple_imaging ; 1 conv_imaging kv (Q, gh, gw, kv) ; 2 w_cache_imaging (wstep, Q = qpx, npixFF, gh = npixKern)
struct ImagingFn {
    int kind;
    int64_t wstep, Q, npixFF, gh, gw;
    const double *kv;
    double theta;
    int64_t lam;
};
// N = the image size; w_cache_imaging's wstep default (2000, :412) is filled in; GRIDHIP_EINVAL for an unknown kind, a
// kind's options out of range or N <= 0.  Which pointers a call needs is its caller's own rule.
int imaging_fn_check(gridhip_ctx *ctx, ImagingFn &fn, int64_t *N);

// What w_cache_imaging (src/Gridding.hs:399-449) derives from the baselines alone: scaled u, v, the
// w-bins and one conjugated w-kernel per plane.  do_imaging calls the imaging function twice with the
// same baselines (image and PSF, :538,541); the reference rebuilds everything both times ("no cache
// despite the name", :405-411) — here the second call reuses it.
struct WCache {
    DevBuf pu, pv, wb;
    double2 *table = nullptr;  // the context's cached table (ImagingState::wk_cache): not owned
    int64_t nplanes = 0;
    bool ready = false;
    gridhip_plan *plan = nullptr;  // the baselines binned once for both passes
    ~WCache() { gridhip_plan_destroy(plan); }
};
// u, v, w: n contiguous doubles each (wavelengths); synchronises (the w-bin rule reads min / max back)
int w_cache_prepare(gridhip_ctx *ctx, WCache &c, double theta, int64_t lam, int64_t wstep, int64_t Q, int64_t npixFF,
                    int64_t S, int64_t n, const double *u, const double *v, const double *w);

// a[k] = 1 + 0i; out[k] = a[k] * b[k] (out may be b): do_imaging's weights and wt * vis1 (src/Gridding.hs:534-538)
int launch_fill_ones(gridhip_ctx *ctx, int64_t n, double2 *a);
int launch_cmul(gridhip_ctx *ctx, int64_t n, const double2 *a, const double2 *b, double2 *out);

// the arguments of the aw entry points (aw_imaging_dev, do_imaging_aw, aw_gridding, predict_aw)
struct AwArgs {
    double theta;
    int64_t lam, W, Q, S, A;
    const double *wkerns, *wvals, *akerns;
    int64_t n;
    const double *u, *v, *w;
    int64_t stride;
    const int64_t *a1, *a2;
    const double *vis;
};
// N = image size; vis_needed: whether the call reads vis (the gridding entry points do, predict_aw does not)
int aw_check(gridhip_ctx *ctx, const AwArgs &a, int64_t *N, bool vis_needed = true);
// The arguments as the kernels see them: a's nine pointers taken through st.in (vis stays null where the entry point
// reads none).  The caller checks st.status() after its own last argument.
AwArgs stage_aw(Staged &st, const AwArgs &a);
// p = uvw1 / lam, w-bins, and (mirror) vis1, (weigh) wt * vis1 in vis1 and (want_wt) wt: aw_front_kernel +
// aw_weight_kernel.  weigh: 0 none, 1 on the mirrored coordinates, 2 on the un-mirrored ones.
struct AwFront {
    DevBuf pu, pv, wb, vis1, wt, cell, cnt;
};
int aw_front(gridhip_ctx *ctx, int64_t N, const AwArgs &d, double fc, bool mirror, int weigh, bool want_wt, AwFront &f);

// ---- deconvolution (clean.hip) -------------------------------------------------------------------------------------------
// (what the four CLEANs share on the device and in their launchers - the tile, the table entry, the search rule, the
// walk over a tile - is in clean_walk.h, which only they include; here are the host declarations)
// the largest N clean's tile grid holds (65535 rows of 16-row tiles); the restore takes the same limit
constexpr int64_t CLEAN_MAX_N = 16 * 65535;
// gridhip_clean's argument rules (GRIDHIP_EINVAL; an N the tile grid cannot hold is GRIDHIP_EUNSUPPORTED)
int clean_check(gridhip_ctx *ctx, int64_t N, const double *psf, const double *residual, const double *model, double gain,
                double threshold, int64_t niter, int64_t border, int64_t patch);
// the state block and the tile table of an N x N clean
size_t clean_scratch_bytes(int64_t N);
// What the _auto forms add to a clean (include/gridhip.h, "masks and noise-based stop levels"): the clean mask, or null;
// T = max(threshold, nsigma * *noise, peak_frac * |first peak|), noise a device pointer; on: stats has the four further
// doubles { T, reason, first peak, 0 }.  The neutral value - what the plain entry points pass - is CleanAuto{}.
struct CleanAuto {
    const uint8_t *mask = nullptr;
    double nsigma = 0.0;
    const double *noise = nullptr;
    double peak_frac = 0.0;
    bool on = false;
};
// the _auto forms' own argument rules (GRIDHIP_EINVAL), after clean_check's
int clean_auto_check(gridhip_ctx *ctx, int64_t N, const double *residual, const double *model, const uint8_t *mask,
                     double nsigma, const double *noise, double peak_frac);
// gridhip_clean_dev / gridhip_clean_auto_dev on checked arguments: kernels only, on ctx->stream; scratch:
// clean_scratch_bytes(N) of device memory
int clean_run(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
              double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch,
              const CleanAuto &au = CleanAuto{});

// ---- multi-scale CLEAN (msclean.hip) ---------------------------------------------------------------------------------------
constexpr int MS_MAX_SCALES = 6;
constexpr double MS_MAX_SCALE = 32.0;
// gridhip_msclean's argument rules: clean's, then the scale list's (GRIDHIP_EINVAL; a scale above 32 cells is
// GRIDHIP_EUNSUPPORTED)
int msclean_check(gridhip_ctx *ctx, int64_t N, const double *psf, const double *residual, const double *model, int64_t S,
                  const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                  int64_t patch);
// the state block, the S tile tables, the taps, the S - 1 smoothed residuals and the S (S + 1) / 2 - 1 cross-PSFs
size_t msclean_scratch_bytes(int64_t N, int64_t S);
// gridhip_msclean_dev on checked arguments: kernels only, on ctx->stream.  setup: make the taps, the pointer table and the
// cross-PSFs of `psf` in scratch; a caller whose scratch holds them for this psf and these scales passes false.
int msclean_run(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                int64_t patch, double *stats, void *scratch, bool setup, const CleanAuto &au = CleanAuto{});

// ---- multi-term CLEAN (mfclean.hip) -----------------------------------------------------------------------------------------
constexpr int MF_MAX_TERMS = 4;
// gridhip_mfclean's argument rules: T in 1 .. 4, then clean's, then no two of the 4T - 1 planes overlapping (GRIDHIP_EINVAL)
int mfclean_check(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, const double *residuals,
                  const double *models, double gain, double threshold, int64_t niter, int64_t border, int64_t patch);
// the state block and the tile table of an N x N multi-term clean, the same for every T
size_t mfclean_scratch_bytes(int64_t N);
// gridhip_mfclean_dev on checked arguments: kernels only, on ctx->stream; scratch: mfclean_scratch_bytes(N)
int mfclean_run(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch);

// ---- joint CLEAN (jclean.hip) -------------------------------------------------------------------------------------------------
constexpr int JC_MAX_PLANES = 8;
// gridhip_jclean's argument rules: P, Q, metric and the weights, then clean's and clean_auto's, then no overlap among the
// Q + 2P planes and the mask (GRIDHIP_EINVAL; clean's GRIDHIP_EUNSUPPORTED limit on N)
int jclean_check(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, const double *residuals,
                 const double *models, const double *weights, int metric, double gain, double threshold, int64_t niter,
                 int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac);
// the state block and the tile table of an N x N joint clean, the same for every P
size_t jclean_scratch_bytes(int64_t N);
// gridhip_jclean_dev on checked arguments: kernels only, on ctx->stream; weights is the host's; scratch: jclean_scratch_bytes(N)
int jclean_run(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals, double *models,
               const double *weights, int metric, double gain, double threshold, int64_t niter, int64_t border,
               int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac, double *stats,
               void *scratch);

// ---- robust image statistics (noise.hip) -----------------------------------------------------------------------------------
// gridhip_image_stats' argument rules (GRIDHIP_EINVAL, GRIDHIP_EUNSUPPORTED)
int image_stats_check(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                      const double *stats);
// the state block, the bin table and one row per work-group; the same for every N
size_t image_stats_scratch_bytes(gridhip_ctx *ctx);
// gridhip_image_stats_dev on checked arguments: kernels only, on ctx->stream
int image_stats_run(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border, double *stats,
                    void *scratch);

// ---- auto-masking (automask.hip) ---------------------------------------------------------------------------------------------
// gridhip_automask's argument rules (GRIDHIP_EINVAL, then GRIDHIP_EUNSUPPORTED); noise is not read (it may live on the device)
int automask_check(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border, double thr_hi,
                   double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                   int64_t min_cells, int64_t grow, const double *stats);
// the state block, one row per work-group, two int32 label planes and a byte plane
size_t automask_scratch_bytes(gridhip_ctx *ctx, int64_t N);
// The head of the scratch block: the levels, the reason (0: the steps run; 2, 3: every kernel after the levels leaves at
// once) and the four counts of the stats.
struct AmState {
    double T_hi, T_lo, P;
    int reason, pad;
    unsigned int nH, nSurv, nKept, nNew;
};
// What steps 1-3 leave in the scratch block: the labels of L (a cell's label is the smallest index of its component, -1
// outside L), a second int32 plane that is free again (0, or 1 at the roots of the kept components) and the bytes of K.
struct AmPlanes {
    AmState *state;
    int *label, *spare;
    uint8_t *kbyte;
};
AmPlanes automask_planes(gridhip_ctx *ctx, int64_t N, void *scratch);
// the rules of N, border, image, min_cells and the levels alone (GRIDHIP_EINVAL), for automask and find_sources (`who`)
int automask_levels_check(gridhip_ctx *ctx, const char *who, int64_t N, const double *image, int64_t border, double thr_hi,
                          double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                          int64_t min_cells);
// steps 1-3 on checked arguments: the first 11 kernels of an automask.  An early end (reason 2, 3) writes the 8 stats
// { T_hi, T_lo, P, 0, 0, 0, 0, reason } and leaves the planes as they were: whoever reads them reads the reason first.
int automask_label_run(gridhip_ctx *ctx, int64_t N, const double *image, int64_t border, int absolute, double thr_hi,
                       double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                       int64_t min_cells, double *stats, void *scratch);
// gridhip_automask_dev on checked arguments: 13 kernels on ctx->stream, nothing else
int automask_run(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                 double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                 int64_t min_cells, int64_t grow, double *stats, void *scratch);

// ---- the restoring beam and the restore (restore.hip) --------------------------------------------------------------------
// gridhip_fit_beam's and gridhip_restore's argument rules (GRIDHIP_EINVAL, GRIDHIP_EUNSUPPORTED); the beam's values are
// not looked at (they may live on the device)
int fit_beam_check(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, const double *beam);
int restore_check(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                  int64_t support, const double *restored);
// the _dev forms on checked arguments: one kernel each on ctx->stream, no scratch
int fit_beam_run(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam);
int restore_run(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                int64_t support, double *restored);
// a beam restore and find_sources may use: ok set, A, B, C finite and positive definite
__host__ __device__ inline bool beam_usable(double A, double B, double C, double ok)
{
    const double inf = __builtin_inf();
    return ok != 0.0 && ok == ok && A > 0.0 && A < inf && C > 0.0 && C < inf && B > -inf && B < inf && A * C - B * B > 0.0;
}
// What restore.hip and msclean.hip's set-up convolution share: the tile and the staged LDS layout (restore.hip's head).
constexpr int RS_TH = 32, RS_TW = 64, RS_LX = RS_TW / 8;  // the tile; lanes along x
// the staged width of `cols` cells (cell u lies at u + u / 8) and the row stride: the next count that is 8 modulo 32
__host__ __device__ inline int staged_pos(int u) { return u + (u >> 3); }
inline int staged_stride(int s)
{
    const int w = staged_pos(RS_TW + 2 * s - 1) + 1;
    return w + ((8 - w % 32) + 32) % 32;
}
inline size_t restore_lds_bytes(int s)
{
    const int K = 2 * s + 1;
    return ((size_t)(RS_TH + 2 * s) * staged_stride(s) + (size_t)K * K) * sizeof(double);
}

// ---- imaging weights (weights.hip) ---------------------------------------------------------------------------------------
// The cell code of a flagged visibility (a data weight that is not > 0); -1 stays "outside the grid".
constexpr int64_t WEIGHT_FLAGGED = -2;
// What the density pass does with one visibility whose doweight cell is c: a flagged one takes part in nothing, an
// unflagged one in the grid adds its data weight to the density (dens, fp64) or, without data weights, 1 to the count
// (cnt); whichever the mode does not need is null.  Returns the cell code the second pass reads.
__device__ __forceinline__ int64_t weight_note(int64_t c, const double *__restrict__ wt_in, int64_t k,
                                               unsigned int *__restrict__ cnt, double *__restrict__ dens)
{
    if (wt_in) {
        const double s = wt_in[k];
        if (!(s > 0.0)) return WEIGHT_FLAGGED;
        if (c >= 0 && dens) atomicAdd(&dens[c], s);
    } else if (c >= 0 && cnt) {
        atomicAdd(&cnt[c], 1u);
    }
    return c;
}
// gridhip_weights' rules for mode, robust and taper_sigma (GRIDHIP_EINVAL)
int weights_mode_check(gridhip_ctx *ctx, int mode, double robust, double sigma);
// The scratch of one weighting: the N x N density (counts without data weights; absent for natural weighting) and the
// accumulators (the two sums over the cells, then one row of partial sums per work-group of the second pass).
struct WeightScratch {
    DevBuf dens, acc;
    unsigned int *cnt = nullptr;  // one of the two views of dens, or neither
    double *den = nullptr;
};
// takes the scratch from the pool and zeroes it with a kernel (no memset node)
int weights_begin(gridhip_ctx *ctx, int64_t N, int mode, bool data_weights, WeightScratch &s);
// Everything after the density pass, kernels only: the sums over the cells (Briggs), the pass that writes the weights and
// the partial sums, and (stats != null) the 8 doubles.  cell: the codes the density pass left, or null - the pass then
// takes the cell of (u / lam, v / lam) itself (natural weighting needs no density pass).  u, v are read for the taper and
// for a null cell only.  keep_sign: out holds +-1 and keeps its sign (an imager's mirror flag).  out may be wt_in.
int weights_finish(gridhip_ctx *ctx, int64_t N, int64_t n, int mode, double robust, double sigma, const int64_t *cell,
                   WeightScratch &s, const double *wt_in, const double *u, const double *v, int64_t stride, double lam,
                   double *out, bool keep_sign, double *stats);

// ---- gain calibration (gaincal.hip) --------------------------------------------------------------------------------------
// the visibilities of one chunk of the iteration kernel (a work-group takes whole chunks); the most antennas whose gains
// and sums of one interval the kernel keeps in LDS (above it the sums go straight to global memory); the most (interval,
// antenna) cells of a solve - and so of A and of T alone, which the packed key's 21-bit fields rely on
constexpr int64_t GC_CHUNK = 4096;
constexpr int GC_LDS_A = 512;
constexpr int64_t GC_MAX_TABLE = (int64_t)1 << 21;
// gridhip_gaincal's and gridhip_apply_gains' argument rules (GRIDHIP_EINVAL, GRIDHIP_EUNSUPPORTED)
int gaincal_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                  const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                  int64_t refant, int64_t niter, double tol, const double *gains);
int apply_gains_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                      const double *vis_out, const double *wt_out);
// the _dev forms on checked arguments: kernels only, on ctx->stream; scratch from the context's pool.  vis_cal != null:
// the final pass also writes apply_gains(inverse = 1) of vis, wt into vis_cal and (when given) wt_cal - a selfcal
int gaincal_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
                int warm, int64_t niter, double tol, double *gains, double *stats, double *vis_cal, double *wt_cal);
int apply_gains_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                    double *vis_out, double *wt_out);

// ---- direction-dependent calibration (ddcal.hip) -----------------------------------------------------------------------------
// the most directions of a solve; the LDS a work-group of the iteration kernel may take for the gains and sums of one
// interval ((D^2 + 4 D) * 8 bytes per antenna: gridhip_ddcal_lds_antennas, include/gridhip.h)
constexpr int DD_MAX_D = 8;
constexpr int64_t DD_LDS_BUDGET = 128 * 1024;
// gridhip_ddcal's and gridhip_dd_subtract's argument rules (GRIDHIP_EINVAL, GRIDHIP_EUNSUPPORTED)
int ddcal_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
                int64_t niter, double tol, const double *gains);
int dd_subtract_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs, const double *vis_in,
                      const double *vis_out);
// what the checks of the calls a peel replaces leave open: row 0 of model_vis is written and may overlap no input and no
// other output (gains and vis_cal are covered by the two checks above), and wt_cal may overlap none of the D x T x A
// (cells) gains, where apply_gains_check sees direction 0 alone
int peel_check(gridhip_ctx *ctx, int64_t n, int64_t cells, const double *model_vis, const double *gains, const int64_t *a1,
               const int64_t *a2, const int64_t *slot, const double *vis, const double *wt, const double *wt_cal,
               const double *stats);
// the _dev forms on checked arguments: kernels only, on ctx->stream; scratch from the context's pool
int ddcal_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
              const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
              int warm, int64_t niter, double tol, double *gains, double *stats);
int dd_subtract_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs, const double *vis_in,
                    double *vis_out);

// ---- polarisation (jonescal.hip) -----------------------------------------------------------------------------------------
// the most antennas whose Jones matrices and sums of one interval the iteration kernel keeps in LDS, 160 bytes each
// (gridhip_jonescal_lds_antennas, include/gridhip.h); the chunk, the table limit and the key are gaincal's
constexpr int JC_LDS_A = 512;

// ---- residual flagging (flag.hip) ------------------------------------------------------------------------------------------
// the most groups of one call (the bin table is 1 KB per group); the most groups whose bins a work-group of the histogram
// keeps in LDS (above it the lanes add to the global table directly); the most clipping rounds
constexpr int64_t FLAG_MAX_GROUPS = (int64_t)1 << 18;
constexpr int FLAG_LDS_GROUPS = 64;
constexpr int FLAG_MAX_ROUNDS = 16;
// gridhip_flag_residuals' argument rules (GRIDHIP_EINVAL, then GRIDHIP_EUNSUPPORTED); nothing is read
int flag_check(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis, const double *model_vis,
               const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter, const double *wt_out,
               const uint8_t *flags_out, const double *group_stats, const double *stats);
// the state block, 40 B and the 1 KB of bins per group, 12 B per visibility
size_t flag_scratch_bytes(int64_t n, int64_t G);
// gridhip_flag_residuals_dev on checked arguments: kernels only, on ctx->stream; scratch: flag_scratch_bytes(n, G)
int flag_run(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis, const double *model_vis,
             const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter, double *wt_out,
             uint8_t *flags_out, double *group_stats, double *stats, void *scratch);
// What time-frequency flagging (sumthreshold.hip) shares with the clip: the front pass and the select, one copy of each.
constexpr unsigned int FLAG_DEAD = 0xffffffffu;  // the group code of a visibility that takes part in nothing
constexpr unsigned int FLAG_LEFT = 0xfffffffeu;  // and of one that is left alone
struct FlagState {  // 256 bytes at the head of the scratch block
    unsigned int clipped[FLAG_MAX_ROUNDS];  // per round; the counter of round r is the stop flag of round r + 1
    unsigned int cls[5];  // participants at the start of round 0, then the visibilities of the classes 1 to 4
    unsigned int sir;     // samples added by the SIR operator (sumthreshold.hip)
    unsigned int pad[42];
};
static_assert(sizeof(FlagState) == 256, "the state block");
struct FlagGroup {  // one row of the per-group state table
    unsigned long long prefix;  // the digits of the wanted key chosen so far (the lower bits zero)
    double med, mad, T;
    unsigned int rank;  // the wanted rank among the participants whose higher digits equal the prefix
    unsigned int n;     // the participants of the group in this round
};
static_assert(sizeof(FlagGroup) == 40, "the per-group state");
struct FlagScratch {  // the parts of a block of flag_scratch_bytes(n, G)
    FlagState *st;
    FlagGroup *gs;
    unsigned int *bins;
    unsigned long long *keys;  // the bits of a_k
    unsigned int *codes;       // the group of a participant, FLAG_DEAD or FLAG_LEFT
};
FlagScratch flag_scratch_parts(void *scratch, int64_t n, int64_t G);
// has round r been stopped?  (round 0 always runs)
__device__ __forceinline__ bool flag_stopped(const FlagState *st, int r) { return r > 0 && st->clipped[r - 1] == 0; }
// the sum of x over the work-group's waves goes to *dst with one integer atomic per wave
__device__ __forceinline__ void flag_wave_count(unsigned int x, unsigned int *dst)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}
// flag_init_kernel and flag_front_kernel.  cube_div > 0: the n samples are a dense cube and the group of sample k is
// (k / cube_div) % G - the baseline of [B][T][F] (cube_div = T F) or of [T][B][F] (cube_div = F); group is not read.
int flag_front(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, int64_t cube_div, const double *vis,
               const double *model_vis, const double *wt_in, double amax, uint8_t *flags_out, const FlagScratch &s);
// The select of round `round`, 32 launches: n_g, med_g and MAD_g of every group into s.gs, and with sigma_g = 1.4826 MAD_g
// T_g = med_g + level * sigma_g, or level * sigma_g alone (sigma_only), or +Inf for a group below min_count or of ties;
// group_stats as gridhip_flag_residuals defines it.  round < 0: the groups' counts alone, 2 launches.
int flag_select(gridhip_ctx *ctx, int64_t n, int64_t G, int round, double level, bool sigma_only, int64_t min_count,
                double *group_stats, const FlagScratch &s);

// ---- time-frequency flagging (sumthreshold.hip) ---------------------------------------------------------------------------
// the stage kernel's tile, the most stages (windows up to 64) and rounds, the longest row
constexpr int ST_TILE_T = 32, ST_TILE_F = 32;
constexpr int ST_MAX_STAGES = 7, ST_MAX_ROUNDS = 4;
constexpr int64_t ST_MAX_ROW = (int64_t)1 << 20;

// ---- direct-Fourier prediction of a component list (dft.hip) ---------------------------------------------------------------
// gridhip_dft_predict's and gridhip_components_from_image's argument rules (GRIDHIP_EINVAL, GRIDHIP_EUNSUPPORTED); *N: the
// image size
int dft_predict_check(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count, int T, int64_t n,
                      const double *u, const double *v, const double *w, int64_t stride, const double *x,
                      const double *vis_sub, const double *vis_out, const double *stats);
int components_check(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model, int64_t max_c,
                     const double *comps, const int64_t *count, int64_t *N);
// the component slices S of a call: the option "dft_slices" when it is set, else a function of (n, C) alone
int dft_slices(gridhip_ctx *ctx, int64_t n, int64_t C);
// the _dev forms on checked arguments: kernels only, on ctx->stream; scratch (80 B per component, 16 S B per visibility
// when S > 1, one row per work-group) from the context's pool
int dft_predict_run(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count_dev, int T, int64_t n,
                    const double *u, const double *v, const double *w, int64_t stride, const double *x,
                    const double *vis_sub, double *vis_out, double *stats);
int components_run(gridhip_ctx *ctx, int64_t N, double theta, int T, const double *model, int64_t max_c, double *comps,
                   int64_t *count_dev);

// What the two ordered compactions (dft.hip's non-zero cells, sources.hip's island roots) share: the counts of the threads
// before this one (exclusive) and of all the work-group of 256 (*total); lds: 4 values
__device__ __forceinline__ unsigned int block_rank(unsigned int mine, unsigned int *lds, unsigned int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned int before = 0, all = 0;
    for (int wv = 0; wv < 4; ++wv) {
        if (wv < wave) before += lds[wv];
        all += lds[wv];
    }
    *total = all;
    return before + inc - mine;
}
constexpr int CFI_SEG = 1024;  // cells of a segment of a compaction: 4 per thread
// offs = the exclusive scan of the nseg segment counts, *count = their sum: one work-group (cfi_scan_kernel, dft.hip)
int segment_scan(gridhip_ctx *ctx, int64_t nseg, const unsigned int *segcount, int64_t *offs, int64_t *count);

// ---- source finding (sources.hip) ---------------------------------------------------------------------------------------------
constexpr int64_t SRC_MAX_N = 46340;  // automask's limit: labels are 32-bit cell indices
constexpr int64_t SRC_MAX_DEBLEND = 32;  // the largest window radius of the option "sources_deblend"
// gridhip_find_sources' argument rules (GRIDHIP_EINVAL, then GRIDHIP_EUNSUPPORTED) and the option's; nothing is read; *N:
// the image size
int sources_check(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                  double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                  int64_t min_cells, const double *beam, int correct, int64_t max_c, const double *comps, const double *info,
                  const int64_t *count, const double *stats, int64_t *N);
// the segment counts and offsets of the compaction, and a root and a box per row that can be written
size_t sources_scratch_bytes(int64_t N, int64_t max_c);
// gridhip_find_sources_dev on checked arguments: kernels only, on ctx->stream; am_scratch: automask_scratch_bytes(N),
// scratch: sources_scratch_bytes(N, max_c).  With the option "sources_deblend" set it takes 16 B per cell more from the
// context's pool for the length of the call
int sources_run(gridhip_ctx *ctx, int64_t N, double theta, const double *image, int64_t border, double thr_hi,
                double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac, int64_t min_cells,
                const double *beam, int correct, int64_t max_c, double *comps, double *info, int64_t *count, double *stats,
                void *am_scratch, void *scratch);

// ---- reprojection and mosaicking (mosaic.hip) ------------------------------------------------------------------------------
// gridhip_mosaic's argument rules (GRIDHIP_EINVAL, then GRIDHIP_EUNSUPPORTED); nothing is read
int mosaic_check(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                 const double *R, int kind, double inner, double outer, double wmin, int64_t Nd, double theta_d,
                 const double *out, const double *wsum, const double *stats);
// the counter block and 80 B per facet (R_f and its verdict)
size_t mosaic_scratch_bytes(int64_t F);
// gridhip_mosaic_dev on checked arguments: kernels only, on ctx->stream; scratch: mosaic_scratch_bytes(F).  R is device
// memory: the prologue kernel judges it
int mosaic_run(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
               const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank, int64_t Nd,
               double theta_d, double *out, double *wsum, double *stats, void *scratch);

// ---- w-stacking (wstack.hip) ------------------------------------------------------------------------------------------------
// the most layers of a stack (the per-layer histogram of the partition is kept in LDS: 2 x 16 KB) and the most planes of a
// layer (w_cache_imaging's limit of one kernel table)
constexpr int64_t WS_MAX_LAYERS = 4096;
constexpr int64_t WS_MAX_PLANES = 65536;
// The arguments a stack is made from, and their rules (GRIDHIP_EINVAL; n or M beyond the limits: GRIDHIP_EUNSUPPORTED).
// Nothing is read.  *N: the image size.
struct WStackArgs {
    int64_t wstep, M, Q, npixFF, S;
    double theta;
    int64_t lam, n;
    const double *u, *v, *w;
    int64_t stride;
};
int wstack_check(gridhip_ctx *ctx, const WStackArgs &a, int64_t *N);
// gridhip_wstack_create_dev on checked arguments (synchronises: the plane range and the layer counts come back).  own_fft:
// the stack keeps a transform of its own (a handle outlives the context's four cached sizes); false: the passes take the
// context's cached one
// What an imager lends the two stacks it holds (imager.hip, the w-stacking kind), and the half of a stack each of them is:
// 1 = the predict passes only (no scatter grid), 2 = the image passes only (no gather grid).  A lent stack builds no
// table and makes no transform: K, conj(K) and the transform are the lender's, which outlives the stack.
struct WsLend {
    int half;
    void *fft;
    double2 *ktab, *ktab_g;
};
int wstack_create(gridhip_ctx *ctx, const WStackArgs &a, int64_t N, gridhip_wstack **out, bool own_fft = true,
                  const WsLend *lend = nullptr);
// ktab = K[M][Q][Q][S][S], the table of the residual planes, and ktab_g = conj(K) (asynchronous)
int wstack_tables(gridhip_ctx *ctx, const WStackArgs &a, double2 *ktab, double2 *ktab_g);
void wstack_release(gridhip_wstack *ws);  // gridhip_wstack_destroy's
// The two passes on device pointers: kernels and transforms only, on the stack's context's stream.
// image = factor * Re(D(vis)), overwritten (factor 1: gridhip_wstack_image_dev; 2: do_imaging, see include/gridhip.h)
int wstack_image_run(gridhip_wstack *ws, const double *vis, double *image, double factor);
int wstack_predict_run(gridhip_wstack *ws, const double *model, const double *vis_sub, double *vis_out);
// The passes without their permuting ends, for a caller that works in layer order itself: the predictions of `model` left
// in the stack's layer-ordered block; the image of what that block holds.
int wstack_predict_layers(gridhip_wstack *ws, const double *model);
int wstack_image_layers(gridhip_wstack *ws, double *image, double factor);
// the visibilities that have a layer
int64_t wstack_count(const gridhip_wstack *ws);
// back[j'] = j where `from` keeps at j the visibility that `to` keeps at j' (wstack_count(to) entries; the two stacks are
// of one stream's visibilities, as an imager's un-mirrored and mirrored ones are).  *same: the two stacks keep the same
// visibilities - always, but for image-domain layers, which drop what lies off the grid of their own stream: then false,
// `back` is not to be used and the caller takes the passes in stream order.  Synchronises for image-domain layers.
int wstack_compose(gridhip_wstack *from, gridhip_wstack *to, int32_t *back, bool *same);
// An imager's cycle middle in the layer order of `to` (ws_middle_kernel, wstack.hip): to's block = the weighted, mirrored
// residual of vis and from's block (from = NULL: of vis alone); vis_res (or NULL, or vis) gets the residual in stream order.
int wstack_middle_run(gridhip_wstack *from, gridhip_wstack *to, const int32_t *back, const double *vis, const double *sw,
                      double *vis_res);
// *maxbits = the maximum of x[0 .. cells) in ordered bits (do_imaging's pmax)
int wstack_image_max(gridhip_ctx *ctx, int64_t cells, const double *x, unsigned long long *maxbits);

}  // namespace gridhip
