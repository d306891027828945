// Imagers: what a major cycle holds (include/gridhip.h, "imagers").  An imager is created once from the baselines and
// the imaging function and turns (model, vis) into the residual image in one asynchronous call:
//     image = do_imaging(vis - predict(model)).image
// Everything that depends on the baselines alone is done at creation: the slice / scale of the strided uvw, the mirror,
// the uniform weights, the w-bins, the kernel tables (in memory of the imager's own), the binning of BOTH record sets -
// the un-mirrored one the prediction gathers on and the mirrored one do_imaging scatters on; the two are not mirror
// images of each other bit for bit (floor(.5 + x), the w-bin rule and findClosest are not odd functions), so neither is
// derived from the other - and the PSF with its maximum.  A cycle is then
//     head kernel + forward FFT of the model -> gather (un-mirrored records) -> imager_middle_kernel ->
//     scatter (mirrored records) -> Hermitian fill + inverse FFT + real part / pmax
// with no pre-pass, no table build, no histogram, no PSF pass, no allocation, no synchronisation and no memset node.
// The gather and the scatter are the tile kernels of the plans (plan.hip, awgrid.hip), which lend their records to the
// launchers; the simple kind has no records and keeps its two coordinate sets instead.
// The w-stacking kind (include/gridhip.h, "imagers") holds two half stacks (wstack.hip) in place of the two plans: the
// un-mirrored one runs predict passes only, the mirrored one image passes only, and they share one kernel table, its
// conjugate and the imager's transform.  Its image is gridhip_do_imaging_wstack's: per layer a scatter, an inverse
// transform and the w-screen, 2 Re of the sum divided by pmax - no Hermitian fill.  Its cycle has a middle pass of its own
// in the mirrored stack's layer order (ws_middle_kernel) besides the generic one in stream order.
// Wide-band imaging ("wide-band imaging" in the header) adds to an imager x = (nu - nu_0) / nu_0 per visibility, the
// 2T - 1 spectral PSFs - each the image of a plain cycle of (x^s, 0) - and a residual-visibility block: an mfs_cycle is one
// transform and gather per model term accumulated into that block, then per term one pass over it (times x^t, conjugate
// where mirrored, times the weight), the scatter and the tail.  An imager without spectral terms runs none of this.
#include <string.h>

#include <new>

#include "common.h"
#include "imaging.h"

namespace gridhip {

// Creation front end: one read of the strided (u, v, w) per visibility.  Writes
//   p = uvw / lam of the un-mirrored baseline (pu, pv: what predict's gathers bin) and of the mirrored one (mu, mv: what
//   do_imaging's scatters bin; mirror_uvw, src/Gridding.hs:551-562: v < 0 negates u, v, w) - true divisions, as
//   scale_kernel's; -(u / lam) and (-u) / lam are the same double, so one division serves both;
//   the mirror flag as the sign of sw (+-1 here; the weighting's second pass, weights.hip, puts the weight's magnitude on
//   it - the default, uniform weighting without data weights, is doweight's ones / count, and a weight of zero keeps its
//   sign bit);
//   doweight's cell of the mirrored p (:531-535) or the code of a flagged visibility, and the density (weight_note);
//   w of both streams (w_cache: the w-bin rule needs the whole stream's min and max first) or their findClosest bins (aw:
//   the reference searches with w in wavelengths, :473-474).
// There is no product or sum here for the compiler to contract; frac_coord_dev switches contraction off itself.
__global__ void __launch_bounds__(256)
    imager_front_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                        int64_t stride, double lam, int64_t N, int64_t nws, const double *__restrict__ ws,
                        double *__restrict__ pu, double *__restrict__ pv, double *__restrict__ mu, double *__restrict__ mv,
                        double *__restrict__ w0, double *__restrict__ w1, int64_t *__restrict__ wb0,
                        int64_t *__restrict__ wb1, double *__restrict__ sw, int64_t *__restrict__ cell,
                        const double *__restrict__ wt_in, unsigned int *__restrict__ cnt, double *__restrict__ dens)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double u0 = u[k * stride], v0 = v[k * stride];
        const bool neg = v0 < 0;
        const double qu = u0 / lam, qv = v0 / lam;
        const double ru = neg ? -qu : qu, rv = neg ? -qv : qv;
        pu[k] = qu;
        pv[k] = qv;
        mu[k] = ru;
        mv[k] = rv;
        sw[k] = neg ? -1.0 : 1.0;
        if (w) {
            const double x0 = w[k * stride], x1 = neg ? -x0 : x0;
            if (w0) {
                w0[k] = x0;
                w1[k] = x1;
            }
            if (wb0) {
                wb0[k] = closest_index(nws, ws, x0);
                wb1[k] = closest_index(nws, ws, x1);
            }
        }
        cell[k] = weight_note(weight_cell(N, ru, rv), wt_in, k, cnt, dens);
    }
}

// the PSF pass's input (src/Gridding.hs:541): the weights as complex numbers
__global__ void __launch_bounds__(256)
    imager_wt_kernel(int64_t n, const double *__restrict__ sw, double2 *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = make_double2(fabs(sw[k]), 0.0);
}

// nd doubles of zeros, 16 bytes per lane (a is 16-byte aligned; an odd last double goes alone): the grid before the
// scatter, the predictions where the gather does not write them all, the image of an imager without visibilities
__global__ void __launch_bounds__(256) imager_zero_kernel(int64_t nd, double *__restrict__ a)
{
    const int64_t pairs = nd / 2, k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t k = k0; k < pairs; k += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<double2 *>(a)[k] = make_double2(0.0, 0.0);
    if (k0 == 0 && (nd & 1)) a[nd - 1] = 0.0;
}

// Cycle middle, the one pass over the visibilities between the gather and the scatter (residual_kernel, a copy,
// mirror_kernel and cmul_real_kernel in the two calls an imager replaces, in their order): r = vis - pred (SUB) or vis;
// vis_res = r when asked; then conj where mirrored, then re and im times the real weight, into the gridder's input -
// which is the prediction's own block: element k is read before it is written, by the same lane.
// vis_res may be vis (an in-place residual): no __restrict__ on either.
template <bool SUB>
__global__ void __launch_bounds__(256)
    imager_middle_kernel(int64_t n, const double2 *vis, double2 *pred, const double *__restrict__ sw, double2 *vis_res)
{
#pragma clang fp contract(off)
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        double2 r = vis[k];
        if (SUB) {
            const double2 p = pred[k];
            r = make_double2(r.x - p.x, r.y - p.y);
        }
        if (vis_res) vis_res[k] = r;
        const double s = sw[k];
        const double a = fabs(s);
        if (signbit(s)) r.y = -r.y;
        pred[k] = a == 0.0 ? make_double2(0.0, 0.0) : make_double2(a * r.x, a * r.y);  // (selected out: vis may be NaN)
    }
}

// ---- wide-band imaging (include/gridhip.h, "wide-band imaging"): x_k = (nu_k - nu_0) / nu_0 per visibility, the powers
// pw_0 = 1, pw_t = pw_{t-1} * x, and a visibility whose x is not finite taking part in nothing
__device__ __forceinline__ double spectral_power(double x, int t)
{
    double pw = 1.0;
    for (int i = 0; i < t; ++i) pw = pw * x;
    return pw;
}

// the visibilities whose cycle image is the spectral PSF P_s: (pw_s(x), 0), and 0 where x is not finite
__global__ void __launch_bounds__(256)
    imager_spectral_vis_kernel(int64_t n, const double *__restrict__ x, int s, double2 *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double xk = x[k];
        out[k] = make_double2(isfinite(xk) ? spectral_power(xk, s) : 0.0, 0.0);
    }
}

// r = vis - sum_q pw_q(x) * predict(models[q]), one prediction at a time, q ascending: FIRST starts r from vis, the later
// ones take their term from r.  A visibility whose x is not finite predicts 0 (selected out: pred may be anything).
template <bool FIRST>
__global__ void __launch_bounds__(256)
    imager_mfs_sub_kernel(int64_t n, const double2 *__restrict__ vis, const double2 *__restrict__ pred,
                          const double *__restrict__ x, int q, double2 *__restrict__ r)
{
#pragma clang fp contract(off)
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        double2 v = FIRST ? vis[k] : r[k];
        const double xk = x[k];
        if (isfinite(xk)) {
            const double pw = spectral_power(xk, q);
            const double2 p = pred[k];
            v = make_double2(v.x - pw * p.x, v.y - pw * p.y);
        }
        r[k] = v;
    }
}

// The pass of term t over the residual visibilities r (imager_middle_kernel's, with the power in front): vis_res = r
// when asked; pw_t(x) * r, conjugated where mirrored, times the weight, into the gridder's input; 0 where the weight is 0
// or x is not finite.  vis_res may be r's own block (the caller's vis): no __restrict__ on either.
__global__ void __launch_bounds__(256)
    imager_mfs_term_kernel(int64_t n, const double2 *r, const double *__restrict__ x, const double *__restrict__ sw, int t,
                           double2 *__restrict__ pred, double2 *vis_res)
{
#pragma clang fp contract(off)
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        double2 v = r[k];
        if (vis_res) vis_res[k] = v;
        const double xk = x[k], s = sw[k];
        const double a = fabs(s), pw = spectral_power(xk, t);
        v = make_double2(pw * v.x, pw * v.y);
        if (signbit(s)) v.y = -v.y;
        pred[k] = (a == 0.0 || !isfinite(xk)) ? make_double2(0.0, 0.0) : make_double2(a * v.x, a * v.y);
    }
}

}  // namespace gridhip

using namespace gridhip;

struct gridhip_imager {
    gridhip_ctx *ctx = nullptr;
    int kind = 0;  // 0 simple, 1 conv, 2 w_cache, 3 aw, 4 w-stacking
    int64_t N = 0, n = 0;
    std::vector<void *> owned;  // every device block below
    double *sw = nullptr;       // [n] weight, negative where the baseline is mirrored
    double2 *pred = nullptr;    // [n] the prediction, then the gridder's input
    double2 *g = nullptr, *f = nullptr, *t = nullptr;  // N x N complex: the scatter's grid; fft_c(model), then the tail's
                                                       // Hermitian grid; the forward transform's scratch (odd N only)
    double *psf = nullptr;                             // N x N, normalised
    unsigned long long *pmaxbits = nullptr;            // the PSF's maximum as divide_kernel reads it
    double pmax = 0.0;
    void *fft = nullptr;  // the imager's own N x N transform
    // simple: p of the un-mirrored and the mirrored stream
    double *pu = nullptr, *pv = nullptr, *mu = nullptr, *mv = nullptr;
    // conv, w_cache: the two record sets and their kernel tables (gather: conj kv / the w_kernels; scatter: kv / their
    // conjugates, on the mirrored stream's planes)
    gridhip_plan *gather = nullptr, *scatter = nullptr;
    double2 *ktab_g = nullptr, *ktab_s = nullptr;
    // aw: the same as aw plans, which hold their batches' kernel tables themselves
    gridhip_aw_plan *aw_gather = nullptr, *aw_scatter = nullptr;
    // w-stacking: the half stack of the un-mirrored stream (predict passes) and of the mirrored one (image passes); they
    // borrow ktab_s = K, ktab_g = conj(K) and fft.  ws_back[j'] = the place in the gather's layer order of the visibility
    // the scatter keeps at j' (the layer-order middle pass)
    gridhip_wstack *ws_gather = nullptr, *ws_scatter = nullptr;
    int32_t *ws_back = nullptr;
    bool clear_pred = false;  // the gather does not write every prediction: they start from zero
    void *clean_scratch = nullptr;  // clean's state block and tile table (clean.hip), made by the first clean
    // msclean's scratch (msclean.hip), made by the first msclean and grown by one that needs more; it keeps the taps and
    // the cross-PSFs of the scale list ms_scales between calls (the PSF never changes)
    void *ms_scratch = nullptr;
    size_t ms_bytes = 0;
    std::vector<double> ms_scales;
    double *beam = nullptr;         // the fitted beam of a restore that does not return it (8 doubles), made by the first
    double *wstats = nullptr;       // the weighting's stats (8 doubles), written at creation
    void *noise_scratch = nullptr;  // image_stats' state block and tables (noise.hip), made by the first image_stats
    void *flag_scratch = nullptr;   // flag's state block, tables and keys (flag.hip), made by the first flag and replaced
    size_t flag_bytes = 0;          // by one with more groups
    double *istats = nullptr;       // the image stats of a deconvolve_auto that does not return them (8 doubles)
    void *am_scratch = nullptr;     // automask's state block and planes (automask.hip), made by the first automask
    double *astats = nullptr;       // the automask stats of a deconvolve_automask that does not return them (8 doubles)
    double theta = 0.0;             // the field of view and the wavelength scale of creation: find_sources' l, m
    int64_t lam = 0;
    void *src_scratch = nullptr;    // find_sources' segment table, roots and boxes (sources.hip), made by the first
    int64_t src_rows = -1;          // find_sources and replaced by one with more rows
    // wide-band imaging, made by set_spectral: the number of Taylor terms (0: none), x per visibility, the residual
    // visibilities of an mfs_cycle, the 2T - 1 spectral PSFs, and mfclean's state block and tile table (mfclean.hip)
    int64_t sp_T = 0;
    double *sp_x = nullptr;
    double2 *sp_r = nullptr;
    double *sp_psfs = nullptr;
    void *mf_scratch = nullptr;
};

namespace {

// Which middle pass a w-stacking imager's cycle takes when the option "wstack_middle" is 0: the one that measured faster
// ("W-stacking: the imager kind").  true: the layer-order pass (ws_middle_kernel); the option's 1 is the other.
constexpr bool WS_MIDDLE_LAYERED = true;

template <typename T>
int own(gridhip_imager *im, T **p, size_t bytes)
{
    void *q = nullptr;
    if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return fail(im->ctx, GRIDHIP_ENOMEM, "imager: %zu bytes", bytes);
    im->owned.push_back(q);
    *p = (T *)q;
    return scratch_prefill(im->ctx, q, bytes ? bytes : 16);
}

// n complex numbers (2 n doubles) of zeros
int zero(gridhip_ctx *ctx, int64_t n, double2 *a)
{
    hipLaunchKernelGGL(imager_zero_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, 2 * n, (double *)a);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// pred = the prediction of `model` on the un-mirrored baselines
int gather(gridhip_imager *im, const double *model)
{
    gridhip_ctx *ctx = im->ctx;
    if (im->kind == 4) return wstack_predict_run(im->ws_gather, model, nullptr, (double *)im->pred);  // (its own transforms)
    GH_CHECK(model_transform_to(ctx, im->N, model, im->f, im->t, im->fft));
    if (im->clear_pred) GH_CHECK(zero(ctx, im->n, im->pred));
    switch (im->kind) {
        case 0:  // (the kept p is u / lam already: a division by 1 is exact)
            return launch_simple_degrid(ctx, im->N, im->N, im->f, im->n, im->pu, im->pv, 1, 1.0, im->pred);
        case 3: return gridhip_aw_plan_degrid_dev(im->aw_gather, (const double *)im->f, (double *)im->pred);
        default:
            return gridhip_plan_degrid_dev(im->gather, (const double *)im->ktab_g, (const double *)im->f,
                                           (double *)im->pred);
    }
}

// g = the imaging function's grid of the values in pred, on the mirrored baselines
int scatter(gridhip_imager *im)
{
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(zero(ctx, im->N * im->N, im->g));
    switch (im->kind) {
        case 0:
            return launch_simple_grid(ctx, im->N, im->N, (double *)im->g, im->n, im->mu, im->mv, 1,
                                      (const double *)im->pred);
        case 3: return gridhip_aw_plan_grid_dev(im->aw_scatter, (const double *)im->pred, (double *)im->g);
        default:
            return gridhip_plan_grid_dev(im->scatter, (const double *)im->ktab_s, (const double *)im->pred,
                                         (double *)im->g);
    }
}

// The image of the values in pred on the mirrored baselines: scatter and the imaging tail, or (w-stacking) the mirrored
// stack's image pass times 2.  maxbits: the image's maximum goes there; divbits: the image is divided by the maximum kept
// there (one of the two is null).
int image_pass(gridhip_imager *im, double *out, unsigned long long *maxbits, const unsigned long long *divbits,
               bool layered = false)
{
    gridhip_ctx *ctx = im->ctx;
    if (im->kind != 4) {
        GH_CHECK(scatter(im));
        return image_tail(ctx, im->N, im->g, im->f, out, maxbits, divbits, im->fft);
    }
    // (layered: the middle pass has left the values in the stack's layer order already)
    if (layered)
        GH_CHECK(wstack_image_layers(im->ws_scatter, out, 2.0));
    else
        GH_CHECK(wstack_image_run(im->ws_scatter, (const double *)im->pred, out, 2.0));
    if (maxbits) GH_CHECK(wstack_image_max(ctx, im->N * im->N, out, maxbits));
    if (divbits) GH_CHECK(launch_divide(ctx, im->N * im->N, out, divbits));  // (as normalise divides)
    return GRIDHIP_OK;
}

struct Kernels {  // conv, w_cache: the imaging function; aw: its Q, the tables and the antennas; the weighting
    ImagingFn fn = {};
    int mode = 1;
    double robust = 0.0, sigma = 0.0;
    const double *wt_in = nullptr;
    int64_t W = 0, S = 0, A = 0;
    const double *wkerns = nullptr, *wvals = nullptr, *akerns = nullptr;
    const int64_t *a1 = nullptr, *a2 = nullptr;
};

// Everything creation does, into *im (the caller destroys it on failure).  Arguments are checked by the callers.
int make(gridhip_imager *im, const Kernels &k, double lam, const double *u, const double *v, const double *w,
         int64_t stride)
{
    gridhip_ctx *ctx = im->ctx;
    const ImagingFn &fn = k.fn;
    const int64_t N = im->N, n = im->n;
    const size_t cells = (size_t)N * N;
    GH_CHECK(own(im, &im->psf, cells * 8));
    GH_CHECK(own(im, &im->pmaxbits, 8));
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(int32_t), ctx->stream));  // nothing dropped so far
    GH_CHECK(own(im, &im->wstats, 64));
    WeightScratch wts;
    GH_CHECK(weights_begin(ctx, N, k.mode, k.wt_in != nullptr, wts));
    if (n == 0) {  // a valid imager: no PSF, and every image is zero
        GH_CHECK(weights_finish(ctx, N, 0, k.mode, k.robust, k.sigma, nullptr, wts, nullptr, u, v, stride, lam, nullptr,
                                true, im->wstats));
        GH_CHECK_HIP(ctx, hipMemsetAsync(im->psf, 0, cells * 8, ctx->stream));
        GH_CHECK_HIP(ctx, hipMemsetAsync(im->pmaxbits, 0, 8, ctx->stream));
        return sync(ctx);
    }
    GH_CHECK(own(im, &im->sw, (size_t)n * 8));
    GH_CHECK(own(im, &im->pred, (size_t)n * 16));
    if (im->kind != 4) {  // (the stacks have the one grid each that their passes use)
        GH_CHECK(own(im, &im->g, cells * 16));
        GH_CHECK(own(im, &im->f, cells * 16));
        if (N % 2 != 0) GH_CHECK(own(im, &im->t, cells * 16));
    }
    GH_CHECK(fft_plan_own(ctx, N, &im->fft));

    // ---- front end: both coordinate sets, the mirror flags, the weights
    DevBuf tp[4], tw[2], tb[2], cell;
    double *p[4];
    for (int i = 0; i < 4; ++i) {
        if (im->kind == 0) {
            GH_CHECK(own(im, &p[i], (size_t)n * 8));
        } else {
            GH_CHECK(tp[i].alloc(ctx, (size_t)n * 8));
            p[i] = tp[i].as<double>();
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (im->kind == 2 || im->kind == 4) GH_CHECK(tw[i].alloc(ctx, (size_t)n * 8));
        if (im->kind == 2 || im->kind == 3) GH_CHECK(tb[i].alloc(ctx, (size_t)n * 8));
    }
    GH_CHECK(cell.alloc(ctx, (size_t)n * 8));
    hipLaunchKernelGGL(imager_front_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, u, v,
                       im->kind >= 2 ? w : (const double *)nullptr, stride, lam, N, k.W, k.wvals, p[0], p[1], p[2], p[3],
                       tw[0].as<double>(), tw[1].as<double>(), im->kind == 3 ? tb[0].as<int64_t>() : (int64_t *)nullptr,
                       im->kind == 3 ? tb[1].as<int64_t>() : (int64_t *)nullptr, im->sw, cell.as<int64_t>(), k.wt_in,
                       wts.cnt, wts.den);
    GH_CHECK_HIP(ctx, hipGetLastError());
    // |sw| = the weight (the sign stays); u^2 + v^2 of the taper is the same on either side of the mirror
    GH_CHECK(weights_finish(ctx, N, n, k.mode, k.robust, k.sigma, cell.as<int64_t>(), wts, k.wt_in, u, v, stride, lam,
                            im->sw, true, im->wstats));

    // ---- kernel tables and the two record sets: the gather's first, so that gridhip_last_dropped and
    // gridhip_aw_last_stats report the mirrored stream, as do_imaging does
    if (im->kind == 0) {
        im->pu = p[0], im->pv = p[1], im->mu = p[2], im->mv = p[3];
    } else if (im->kind == 1) {
        const size_t el = (size_t)fn.Q * fn.Q * fn.gh * fn.gw;
        GH_CHECK(own(im, &im->ktab_g, el * 16));
        GH_CHECK(own(im, &im->ktab_s, el * 16));
        GH_CHECK(launch_conj_copy(ctx, (int64_t)el, (const double2 *)fn.kv, im->ktab_g));
        GH_CHECK(copy_in(ctx, im->ktab_s, fn.kv, el * 16, true));
        GH_CHECK(gridhip_plan_create_dev(ctx, N, N, n, 1, fn.Q, fn.gh, fn.gw, p[0], p[1], 1, nullptr, &im->gather));
        GH_CHECK(gridhip_plan_create_dev(ctx, N, N, n, 1, fn.Q, fn.gh, fn.gw, p[2], p[3], 1, nullptr, &im->scatter));
    } else if (im->kind == 2) {
        // the w-bin rule on each stream: its own minimum and plane count, hence a table of its own.  (The gather's
        // planes are the w_kernels, the scatter's their conjugates, :441: two tables even where the ranges agree.)
        int64_t wmin[2] = {0, 0}, np[2] = {0, 0};
        for (int i = 0; i < 2; ++i) {
            GH_CHECK(dev_wbins(ctx, n, tw[i].as<double>(), 1, fn.wstep, tb[i].as<int64_t>(), &wmin[i], &np[i]));
            if (np[i] < 1 || np[i] > 65536) return fail(ctx, GRIDHIP_EUNSUPPORTED, "%lld w-planes", (long long)np[i]);
        }
        const size_t pl = (size_t)fn.Q * fn.Q * fn.gh * fn.gh;
        GH_CHECK(own(im, &im->ktab_g, np[0] * pl * 16));
        GH_CHECK(own(im, &im->ktab_s, np[1] * pl * 16));
        GH_CHECK(build_w_planes(ctx, fn.theta, fn.wstep, wmin[0], np[0], fn.npixFF, fn.gh, fn.Q, im->ktab_g, false));
        GH_CHECK(build_w_planes(ctx, fn.theta, fn.wstep, wmin[1], np[1], fn.npixFF, fn.gh, fn.Q, im->ktab_s, true));
        GH_CHECK(gridhip_plan_create_dev(ctx, N, N, n, np[0], fn.Q, fn.gh, fn.gh, p[0], p[1], 1, tb[0].as<int64_t>(),
                                         &im->gather));
        GH_CHECK(gridhip_plan_create_dev(ctx, N, N, n, np[1], fn.Q, fn.gh, fn.gh, p[2], p[3], 1, tb[1].as<int64_t>(),
                                         &im->scatter));
    } else if (im->kind == 4) {
        // one table K of the residual planes and its conjugate for both stacks; a stack on each stream, the gather's
        // first.  The stacks divide by lam themselves: p is u / lam already, and a division by 1 is exact.
        const size_t tab = (size_t)fn.gw * fn.Q * fn.Q * fn.gh * fn.gh;
        GH_CHECK(own(im, &im->ktab_g, tab * 16));
        GH_CHECK(own(im, &im->ktab_s, tab * 16));
        WStackArgs a{fn.wstep, fn.gw, fn.Q, fn.npixFF, fn.gh, fn.theta, 1, n, p[0], p[1], tw[0].as<double>(), 1};
        GH_CHECK(wstack_tables(ctx, a, im->ktab_s, im->ktab_g));
        WsLend lend{1, im->fft, im->ktab_s, im->ktab_g};
        GH_CHECK(wstack_create(ctx, a, N, &im->ws_gather, false, &lend));
        a.u = p[2], a.v = p[3], a.w = tw[1].as<double>();
        lend.half = 2;
        GH_CHECK(wstack_create(ctx, a, N, &im->ws_scatter, false, &lend));
        GH_CHECK(own(im, &im->ws_back, (size_t)wstack_count(im->ws_scatter) * 4));
        bool same = true;
        GH_CHECK(wstack_compose(im->ws_gather, im->ws_scatter, im->ws_back, &same));
        if (!same) im->ws_back = nullptr;  // (image-domain layers only: every cycle takes the stream-order middle)
    } else {
        // the gather's kernels are conj(aw_kernel_fn2(conj wk, conj ak)) (predict_aw); the aw plans keep what they build
        const size_t wel = (size_t)k.W * fn.Q * fn.Q * k.S * k.S, ael = (size_t)k.A * k.S * k.S;
        DevBuf cwk, cak;
        GH_CHECK(cwk.alloc(ctx, wel * 16));
        GH_CHECK(cak.alloc(ctx, ael * 16));
        GH_CHECK(launch_conj_copy(ctx, (int64_t)wel, (const double2 *)k.wkerns, cwk.as<double2>()));
        GH_CHECK(launch_conj_copy(ctx, (int64_t)ael, (const double2 *)k.akerns, cak.as<double2>()));
        GH_CHECK(gridhip_aw_plan_create_dev(ctx, N, N, n, k.W, fn.Q, k.S, k.A, cwk.as<double>(), cak.as<double>(), p[0],
                                            p[1], 1, tb[0].as<int64_t>(), k.a1, k.a2, &im->aw_gather));
        int64_t tables = ctx->aw_tables_built;
        GH_CHECK(gridhip_aw_plan_create_dev(ctx, N, N, n, k.W, fn.Q, k.S, k.A, k.wkerns, k.akerns, p[2], p[3], 1,
                                            tb[1].as<int64_t>(), k.a1, k.a2, &im->aw_scatter));
        ctx->aw_tables_built += tables;
    }
    if (im->gather) im->clear_pred = plan_caller_clears(im->gather);
    if (im->aw_gather) im->clear_pred = aw_plan_caller_clears(im->aw_gather);
    const int64_t tables = ctx->aw_tables_built;

    // (w-stacking: the gather of an empty model, see below, comes first - its model is the PSF's block while that is
    // still free, and gridhip_last_dropped is left with the mirrored stack's total, which the image pass reports)
    if (im->kind == 4) {
        hipLaunchKernelGGL(imager_zero_kernel, grid_for(ctx, (int64_t)cells / 2 + 1), dim3(256), 0, ctx->stream,
                           (int64_t)cells, im->psf);
        GH_CHECK_HIP(ctx, hipGetLastError());
        GH_CHECK(gather(im, im->psf));
    }
    // ---- the PSF (src/Gridding.hs:541-548) and its maximum
    hipLaunchKernelGGL(imager_wt_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, im->sw, im->pred);
    GH_CHECK_HIP(ctx, hipGetLastError());
    GH_CHECK(image_pass(im, im->psf, im->pmaxbits, nullptr));
    GH_CHECK(launch_divide(ctx, (int64_t)cells, im->psf, im->pmaxbits));
    // one gather of an empty grid: a support the gather cannot hold is refused here, not in the first cycle, and the
    // launchers' scratch has its size before a cycle is captured
    if (im->kind != 4) {  // (w-stacking: done above)
        GH_CHECK(zero(ctx, (int64_t)cells, im->f));
        if (im->clear_pred) GH_CHECK(zero(ctx, n, im->pred));
        if (im->kind == 0)
            GH_CHECK(launch_simple_degrid(ctx, N, N, im->f, n, im->pu, im->pv, 1, 1.0, im->pred));
        else if (im->kind == 3)
            GH_CHECK(gridhip_aw_plan_degrid_dev(im->aw_gather, (const double *)im->f, (double *)im->pred));
        else
            GH_CHECK(gridhip_plan_degrid_dev(im->gather, (const double *)im->ktab_g, (const double *)im->f,
                                             (double *)im->pred));
    }
    ctx->aw_tables_built = tables;  // (the passes above reset it: it reports the creation)
    unsigned long long mb = 0;
    GH_CHECK(d2h(ctx, &mb, im->pmaxbits, 8));
    GH_CHECK(sync(ctx));  // the inputs may be freed or overwritten once this returns
    im->pmax = ordered_value(mb);
    return GRIDHIP_OK;
}

int create(gridhip_ctx *ctx, int kind, int64_t N, int64_t n, const Kernels &k, double lam, const double *u,
           const double *v, const double *w, int64_t stride, gridhip_imager **out)
{
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    gridhip_imager *im = new (std::nothrow) gridhip_imager();
    if (!im) return GRIDHIP_ENOMEM;
    im->ctx = ctx;
    im->kind = kind;
    im->N = N;
    im->n = n;
    const int rc = make(im, k, lam, u, v, w, stride);
    if (rc != GRIDHIP_OK) {
        const std::string why = ctx->err;  // (destroy synchronises: keep the message of the failure)
        gridhip_imager_destroy(im);
        ctx->err = why;
        return rc;
    }
    *out = im;
    return GRIDHIP_OK;
}

}  // namespace

extern "C" {

int gridhip_imager_create_weighted_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh,
                                       int64_t gw, const double *kv, double theta, int64_t lam, int64_t n, const double *u,
                                       const double *v, const double *w, int64_t uv_stride, int mode, double robust,
                                       double taper_sigma, const double *wt_in, gridhip_imager **imager)
{
    if (imager) *imager = nullptr;
    if (!ctx) return GRIDHIP_EINVAL;
    Kernels k;
    k.fn = {kind, wstep, Q, npixFF, gh, kind == 2 ? gh : gw, kv, theta, lam};
    k.mode = mode, k.robust = robust, k.sigma = taper_sigma, k.wt_in = wt_in;
    int64_t N = 0;
    if (kind == 4)  // w-stacking: gw = the planes per layer, and the stack's own rules and limits
        GH_CHECK(wstack_check(ctx, WStackArgs{wstep, gw, Q, npixFF, gh, theta, lam, n, u, v, w, uv_stride}, &N));
    else
        GH_CHECK(imaging_fn_check(ctx, k.fn, &N));
    GH_CHECK(weights_mode_check(ctx, mode, robust, taper_sigma));
    if (!imager || n < 0 || uv_stride < 1 || (n > 0 && (!u || !v || (kind == 2 && !w))))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    if (n > (int64_t)0x7fffff00) return fail(ctx, GRIDHIP_EUNSUPPORTED, "n must be < 2^31 per imager");
    GH_CHECK(create(ctx, kind, N, n, k, (double)lam, u, v, w, uv_stride, imager));
    (*imager)->theta = theta, (*imager)->lam = lam;
    return GRIDHIP_OK;
}

int gridhip_imager_create_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh,
                              int64_t gw, const double *kv, double theta, int64_t lam, int64_t n, const double *u,
                              const double *v, const double *w, int64_t uv_stride, gridhip_imager **imager)
{
    return gridhip_imager_create_weighted_dev(ctx, kind, wstep, Q, npixFF, gh, gw, kv, theta, lam, n, u, v, w, uv_stride, 1,
                                              0.0, 0.0, nullptr, imager);
}

int gridhip_imager_create_aw_weighted_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                                          int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                                          int64_t n, const double *u, const double *v, const double *w,
                                          int64_t uv_stride, const int64_t *a1, const int64_t *a2, int mode, double robust,
                                          double taper_sigma, const double *wt_in, gridhip_imager **imager)
{
    if (imager) *imager = nullptr;
    if (!ctx) return GRIDHIP_EINVAL;
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, nullptr};
    int64_t N = 0;
    GH_CHECK(aw_check(ctx, a, &N, false));
    GH_CHECK(weights_mode_check(ctx, mode, robust, taper_sigma));
    if (!imager) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    // (the aw plans' limits, checked before anything is allocated)
    if (S > 63 || A > 46340 || n > (int64_t)0x7fffff00 || W * Q * Q >= ((int64_t)1 << 30))
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "shape outside aw limits");
    Kernels k;
    k.fn.Q = Q, k.W = W, k.S = S, k.A = A, k.wkerns = wkerns, k.wvals = wvals, k.akerns = akerns, k.a1 = a1, k.a2 = a2;
    k.mode = mode, k.robust = robust, k.sigma = taper_sigma, k.wt_in = wt_in;
    GH_CHECK(create(ctx, 3, N, n, k, (double)lam, u, v, w, uv_stride, imager));
    (*imager)->theta = theta, (*imager)->lam = lam;
    return GRIDHIP_OK;
}

int gridhip_imager_create_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S,
                                 int64_t A, const double *wkerns, const double *wvals, const double *akerns,
                                 int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                                 const int64_t *a1, const int64_t *a2, gridhip_imager **imager)
{
    return gridhip_imager_create_aw_weighted_dev(ctx, theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride,
                                                 a1, a2, 1, 0.0, 0.0, nullptr, imager);
}

int gridhip_imager_weight_stats_dev(gridhip_imager *im, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (!stats) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return copy_out(ctx, stats, im->wstats, 64, true);
}

int gridhip_imager_psf_dev(gridhip_imager *im, double *psf, double *pmax)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (psf) GH_CHECK(copy_out(ctx, psf, im->psf, (size_t)im->N * im->N * 8, true));
    if (pmax) *pmax = im->pmax;
    return GRIDHIP_OK;
}

int gridhip_imager_cycle_dev(gridhip_imager *im, const double *model, const double *vis, double *image, double *vis_res)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    const int64_t n = im->n, cells = im->N * im->N;
    if (!image || (n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        hipLaunchKernelGGL(imager_zero_kernel, grid_for(ctx, cells / 2), dim3(256), 0, ctx->stream, cells, image);
        GH_CHECK_HIP(ctx, hipGetLastError());
        return GRIDHIP_OK;
    }
    mark(ctx, 0);
    // w-stacking: the middle pass in the mirrored stack's layer order, between the layers' gathers and the layers' scatters
    // - or (option "wstack_middle" = 1) the generic one below, in stream order between the stacks' two permuting passes
    if (im->kind == 4 && im->ws_back && (ctx->img->wstack_middle != 0) != WS_MIDDLE_LAYERED) {
        if (model) GH_CHECK(wstack_predict_layers(im->ws_gather, model));
        GH_CHECK(wstack_middle_run(model ? im->ws_gather : nullptr, im->ws_scatter, im->ws_back, vis, im->sw, vis_res));
        mark(ctx, 1);
        GH_CHECK(image_pass(im, image, nullptr, im->pmaxbits, true));
        mark(ctx, 2);
        return GRIDHIP_OK;
    }
    if (model) GH_CHECK(gather(im, model));
    if (model)
        hipLaunchKernelGGL(imager_middle_kernel<true>, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (const double2 *)vis,
                           im->pred, im->sw, (double2 *)vis_res);
    else
        hipLaunchKernelGGL(imager_middle_kernel<false>, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (const double2 *)vis,
                           im->pred, im->sw, (double2 *)vis_res);
    GH_CHECK_HIP(ctx, hipGetLastError());
    mark(ctx, 1);
    GH_CHECK(image_pass(im, image, nullptr, im->pmaxbits));
    mark(ctx, 2);
    return GRIDHIP_OK;
}

int gridhip_imager_predict_dev(gridhip_imager *im, const double *model, const double *vis_sub, double *vis_out)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (!model || (im->n > 0 && !vis_out)) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (im->n == 0) return GRIDHIP_OK;
    GH_CHECK(gather(im, model));
    return launch_residual(ctx, im->n, im->pred, (const double2 *)vis_sub, (double2 *)vis_out);
}

// predict -> gaincal -> apply_gains(inverse = 1) as one enqueued chain (gaincal.hip): the solver reads the prediction where
// the gather left it, and the solve's final pass writes the corrected stream
int gridhip_imager_selfcal_dev(gridhip_imager *im, const double *model, const double *vis, int64_t A, int64_t T,
                               const int64_t *a1, const int64_t *a2, const int64_t *slot, const double *wt, int mode,
                               int64_t refant, int warm, int64_t niter, double tol, double *gains, double *vis_cal,
                               double *wt_cal, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    const int64_t n = im->n;
    if (!model) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK(gaincal_check(ctx, n, A, T, a1, a2, slot, vis, (const double *)im->pred, wt, mode, refant, niter, tol, gains));
    GH_CHECK(apply_gains_check(ctx, n, A, T, a1, a2, slot, gains, 1, vis, wt, vis_cal, wt_cal));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (n > 0) GH_CHECK(gather(im, model));
    return gaincal_run(ctx, n, A, T, a1, a2, slot, vis, (const double *)im->pred, wt, mode, refant, warm, niter, tol, gains,
                       stats, vis_cal, wt_cal);
}

// predict -> ddcal -> dd_subtract(directions 1 .. D - 1) -> apply_gains(gains[0], inverse = 1) as one enqueued chain
// (ddcal.hip): the prediction goes to row 0 of the caller's model_vis, and the stream is corrected in place in vis_cal
int gridhip_imager_peel_dev(gridhip_imager *im, const double *model, const double *vis, int64_t A, int64_t T, int64_t D,
                            const int64_t *a1, const int64_t *a2, const int64_t *slot, const double *wt, int mode,
                            int64_t refant, int warm, int64_t niter, double tol, double *model_vis, double *gains,
                            double *vis_cal, double *wt_cal, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    const int64_t n = im->n;
    if (!model) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK(ddcal_check(ctx, n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, niter, tol, gains));
    const int64_t others = ((int64_t)1 << D) - 2;  // every direction but 0
    GH_CHECK(dd_subtract_check(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, others, vis, vis_cal));
    GH_CHECK(apply_gains_check(ctx, n, A, T, a1, a2, slot, gains, 1, vis, wt, vis_cal, wt_cal));
    GH_CHECK(peel_check(ctx, n, D * A * T, model_vis, gains, a1, a2, slot, vis, wt, wt_cal, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        GH_CHECK(gather(im, model));
        GH_CHECK(launch_residual(ctx, n, im->pred, nullptr, (double2 *)model_vis));
    }
    GH_CHECK(ddcal_run(ctx, n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats));
    GH_CHECK(dd_subtract_run(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, others, vis, vis_cal));
    return apply_gains_run(ctx, n, A, T, a1, a2, slot, gains, 1, vis_cal, wt, vis_cal, wt_cal);
}

// predict -> flag_residuals as one enqueued chain (flag.hip): the front pass reads the prediction where the gather left it
int gridhip_imager_flag_dev(gridhip_imager *im, const double *model, const double *vis, int64_t G, const int64_t *group,
                            const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter,
                            double *wt_out, uint8_t *flags_out, double *group_stats, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    const int64_t n = im->n;
    if (!model) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK(flag_check(ctx, n, G, group, vis, (const double *)im->pred, wt_in, nsigma, amax, min_count, niter, wt_out,
                        flags_out, group_stats, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t need = flag_scratch_bytes(n, G);
    if (need > im->flag_bytes) {
        GH_CHECK(own(im, &im->flag_scratch, need));
        im->flag_bytes = need;
    }
    if (n > 0) GH_CHECK(gather(im, model));
    return flag_run(ctx, n, G, group, vis, (const double *)im->pred, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out,
                    group_stats, stats, im->flag_scratch);
}

static int imager_clean(gridhip_imager *im, double *residual, double *model, double gain, double threshold,
                        int64_t niter, int64_t border, int64_t patch, double *stats, const CleanAuto &au)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(clean_check(ctx, im->N, im->psf, residual, model, gain, threshold, niter, border, patch));
    if (au.on) GH_CHECK(clean_auto_check(ctx, im->N, residual, model, au.mask, au.nsigma, au.noise, au.peak_frac));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!im->clean_scratch) GH_CHECK(own(im, &im->clean_scratch, clean_scratch_bytes(im->N)));
    return clean_run(ctx, im->N, im->psf, residual, model, gain, threshold, niter, border, patch, stats,
                     im->clean_scratch, au);
}

int gridhip_imager_clean_dev(gridhip_imager *im, double *residual, double *model, double gain, double threshold,
                             int64_t niter, int64_t border, int64_t patch, double *stats)
{
    return imager_clean(im, residual, model, gain, threshold, niter, border, patch, stats, CleanAuto{});
}

int gridhip_imager_clean_auto_dev(gridhip_imager *im, double *residual, double *model, double gain, double threshold,
                                  int64_t niter, int64_t border, int64_t patch, const uint8_t *mask, double nsigma,
                                  const double *noise, double peak_frac, double *stats)
{
    return imager_clean(im, residual, model, gain, threshold, niter, border, patch, stats,
                        CleanAuto{mask, nsigma, noise, peak_frac, true});
}

int gridhip_imager_image_stats_dev(gridhip_imager *im, const double *image, const uint8_t *mask, int64_t border,
                                   double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(image_stats_check(ctx, im->N, image, mask, border, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!im->noise_scratch) GH_CHECK(own(im, &im->noise_scratch, image_stats_scratch_bytes(ctx)));
    return image_stats_run(ctx, im->N, image, mask, border, stats, im->noise_scratch);
}

// the checks and the loop the two _auto deconvolves share; minor(c, noise): the c-th minor cycle with sigma at `noise`
extern "C++" template <typename Minor>
static int deconvolve_auto(gridhip_imager *im, const double *vis, double *model, double *image, int64_t nmajor,
                           int64_t border, const uint8_t *mask, double nsigma, double peak_frac, double *istats,
                           Minor minor)
{
    gridhip_ctx *ctx = im->ctx;
    double placeholder = 0.0;  // (stands for sigma's cell in the checks: the loop passes its own)
    GH_CHECK(clean_auto_check(ctx, im->N, image, model, mask, nsigma, &placeholder, peak_frac));
    if (!istats) {
        GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
        if (!im->istats) GH_CHECK(own(im, &im->istats, 64));
    }
    for (int64_t c = 0; c < nmajor; ++c) {
        double *ist = istats ? istats + 8 * c : im->istats;
        GH_CHECK(gridhip_imager_cycle_dev(im, model, vis, image, nullptr));
        GH_CHECK(gridhip_imager_image_stats_dev(im, image, nullptr, border, ist));
        GH_CHECK(minor(c, (const double *)(ist + 3)));
    }
    return gridhip_imager_cycle_dev(im, model, vis, image, nullptr);
}

int gridhip_imager_deconvolve_auto_dev(gridhip_imager *im, const double *vis, double *model, double *image,
                                       int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                       int64_t patch, const uint8_t *mask, double nsigma, double peak_frac,
                                       double *stats, double *istats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "deconvolve: bad argument");
    GH_CHECK(clean_check(ctx, im->N, im->psf, image, model, gain, threshold, niter, border, patch));
    return deconvolve_auto(im, vis, model, image, nmajor, border, mask, nsigma, peak_frac, istats,
                           [&](int64_t c, const double *noise) {
                               return gridhip_imager_clean_auto_dev(im, image, model, gain, threshold, niter, border, patch,
                                                                    mask, nsigma, noise, peak_frac,
                                                                    stats ? stats + 8 * c : nullptr);
                           });
}

int gridhip_imager_deconvolve_dev(gridhip_imager *im, const double *vis, double *model, double *image, int64_t nmajor,
                                  double gain, double threshold, int64_t niter, int64_t border, int64_t patch,
                                  double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "deconvolve: bad argument");
    GH_CHECK(clean_check(ctx, im->N, im->psf, image, model, gain, threshold, niter, border, patch));
    for (int64_t c = 0; c < nmajor; ++c) {
        GH_CHECK(gridhip_imager_cycle_dev(im, model, vis, image, nullptr));
        GH_CHECK(gridhip_imager_clean_dev(im, image, model, gain, threshold, niter, border, patch,
                                          stats ? stats + 4 * c : nullptr));
    }
    return gridhip_imager_cycle_dev(im, model, vis, image, nullptr);
}

// ---- wide-band imaging ---------------------------------------------------------------------------------------------------
// hands a block of the imager's back (hipFree waits for the work that uses it)
static void disown(gridhip_imager *im, void *q)
{
    if (!q) return;
    for (void *&p : im->owned)
        if (p == q) p = nullptr;
    (void)hipFree(q);
}

int gridhip_imager_set_spectral_dev(gridhip_imager *im, int64_t T, const double *x)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (T < 1 || T > MF_MAX_TERMS || (im->n > 0 && !x)) return fail(ctx, GRIDHIP_EINVAL, "set_spectral: bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = im->n, cells = im->N * im->N;
    if (T > im->sp_T) {  // (the first call, or more terms than before)
        disown(im, im->sp_psfs);
        im->sp_psfs = nullptr;
        im->sp_T = 0;
        GH_CHECK(own(im, &im->sp_psfs, (size_t)(2 * T - 1) * cells * 8));
    }
    im->sp_T = 0;  // (a call that fails half way leaves an imager without terms)
    if (!im->sp_x) GH_CHECK(own(im, &im->sp_x, (size_t)n * 8));
    if (!im->sp_r) GH_CHECK(own(im, &im->sp_r, (size_t)n * 16));
    GH_CHECK(copy_in(ctx, im->sp_x, x, (size_t)n * 8, true));
    // P_s = the image of cycle(NULL, (pw_s(x), 0)): the weighted PSF pass with x^s, divided by the stored pmax
    for (int64_t s = 0; s < 2 * T - 1; ++s) {
        if (n > 0) {
            hipLaunchKernelGGL(imager_spectral_vis_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, im->sp_x, (int)s,
                               im->sp_r);
            GH_CHECK_HIP(ctx, hipGetLastError());
        }
        GH_CHECK(gridhip_imager_cycle_dev(im, nullptr, (const double *)im->sp_r, im->sp_psfs + s * cells, nullptr));
    }
    GH_CHECK(sync(ctx));  // x may be freed or overwritten once this returns
    im->sp_T = T;
    return GRIDHIP_OK;
}

int gridhip_imager_spectral_psfs_dev(gridhip_imager *im, double *psfs)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (!im->sp_T || !psfs) return fail(ctx, GRIDHIP_EINVAL, "spectral_psfs: no spectral terms, or a null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return copy_out(ctx, psfs, im->sp_psfs, (size_t)(2 * im->sp_T - 1) * im->N * im->N * 8, true);
}

int gridhip_imager_mfs_cycle_dev(gridhip_imager *im, const double *models, const double *vis, double *images,
                                 double *vis_res)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    const int64_t n = im->n, cells = im->N * im->N, T = im->sp_T;
    if (!T) return fail(ctx, GRIDHIP_EINVAL, "mfs_cycle: the imager has no spectral terms (set_spectral)");
    if (!images || (n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        hipLaunchKernelGGL(imager_zero_kernel, grid_for(ctx, T * cells / 2), dim3(256), 0, ctx->stream, T * cells, images);
        GH_CHECK_HIP(ctx, hipGetLastError());
        return GRIDHIP_OK;
    }
    mark(ctx, 0);
    const double2 *r = (const double2 *)vis;
    if (models) {
        for (int64_t q = 0; q < T; ++q) {
            GH_CHECK(gather(im, models + q * cells));
            if (q == 0)
                hipLaunchKernelGGL(imager_mfs_sub_kernel<true>, grid_for(ctx, n), dim3(256), 0, ctx->stream, n,
                                   (const double2 *)vis, (const double2 *)im->pred, (const double *)im->sp_x, (int)q, im->sp_r);
            else
                hipLaunchKernelGGL(imager_mfs_sub_kernel<false>, grid_for(ctx, n), dim3(256), 0, ctx->stream, n,
                                   (const double2 *)vis, (const double2 *)im->pred, (const double *)im->sp_x, (int)q, im->sp_r);
            GH_CHECK_HIP(ctx, hipGetLastError());
        }
        r = im->sp_r;
    }
    mark(ctx, 1);
    for (int64_t t = 0; t < T; ++t) {
        hipLaunchKernelGGL(imager_mfs_term_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, r,
                           (const double *)im->sp_x, (const double *)im->sw, (int)t, im->pred,
                           t == 0 ? (double2 *)vis_res : (double2 *)nullptr);
        GH_CHECK_HIP(ctx, hipGetLastError());
        GH_CHECK(image_pass(im, images + t * cells, nullptr, im->pmaxbits));
    }
    mark(ctx, 2);
    return GRIDHIP_OK;
}

int gridhip_imager_mfclean_dev(gridhip_imager *im, double *residuals, double *models, double gain, double threshold,
                               int64_t niter, int64_t border, int64_t patch, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (!im->sp_T) return fail(ctx, GRIDHIP_EINVAL, "mfclean: the imager has no spectral terms (set_spectral)");
    GH_CHECK(mfclean_check(ctx, im->N, im->sp_T, im->sp_psfs, residuals, models, gain, threshold, niter, border, patch));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!im->mf_scratch) GH_CHECK(own(im, &im->mf_scratch, mfclean_scratch_bytes(im->N)));
    return mfclean_run(ctx, im->N, im->sp_T, im->sp_psfs, residuals, models, gain, threshold, niter, border, patch, stats,
                       im->mf_scratch);
}

int gridhip_imager_mfdeconvolve_dev(gridhip_imager *im, const double *vis, double *models, double *images, int64_t nmajor,
                                    double gain, double threshold, int64_t niter, int64_t border, int64_t patch,
                                    double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (!im->sp_T) return fail(ctx, GRIDHIP_EINVAL, "mfdeconvolve: the imager has no spectral terms (set_spectral)");
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "mfdeconvolve: bad argument");
    GH_CHECK(mfclean_check(ctx, im->N, im->sp_T, im->sp_psfs, images, models, gain, threshold, niter, border, patch));
    for (int64_t c = 0; c < nmajor; ++c) {
        GH_CHECK(gridhip_imager_mfs_cycle_dev(im, models, vis, images, nullptr));
        GH_CHECK(gridhip_imager_mfclean_dev(im, images, models, gain, threshold, niter, border, patch,
                                            stats ? stats + 8 * c : nullptr));
    }
    return gridhip_imager_mfs_cycle_dev(im, models, vis, images, nullptr);
}

static int imager_msclean(gridhip_imager *im, double *residual, double *model, int64_t S, const double *scales,
                          const double *bias, double gain, double threshold, int64_t niter, int64_t border, int64_t patch,
                          double *stats, const CleanAuto &au)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(msclean_check(ctx, im->N, im->psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch));
    if (au.on) GH_CHECK(clean_auto_check(ctx, im->N, residual, model, au.mask, au.nsigma, au.noise, au.peak_frac));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t need = msclean_scratch_bytes(im->N, S);
    if (need > im->ms_bytes) {  // (the first call, or a longer scale list: hipFree waits for the work that uses the old block)
        if (im->ms_scratch) {
            for (void *&p : im->owned)
                if (p == im->ms_scratch) p = nullptr;
            (void)hipFree(im->ms_scratch);
            im->ms_scratch = nullptr;
        }
        im->ms_bytes = 0;
        im->ms_scales.clear();
        GH_CHECK(own(im, &im->ms_scratch, need));
        im->ms_bytes = need;
    }
    const std::vector<double> key(scales, scales + S);
    const bool setup = key != im->ms_scales;
    im->ms_scales.clear();  // (a set-up that fails half way leaves no key behind)
    GH_CHECK(msclean_run(ctx, im->N, im->psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats,
                         im->ms_scratch, setup, au));
    im->ms_scales = key;
    return GRIDHIP_OK;
}

int gridhip_imager_msclean_dev(gridhip_imager *im, double *residual, double *model, int64_t S, const double *scales,
                               const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                               int64_t patch, double *stats)
{
    return imager_msclean(im, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats, CleanAuto{});
}

int gridhip_imager_msclean_auto_dev(gridhip_imager *im, double *residual, double *model, int64_t S, const double *scales,
                                    const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                                    int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                                    double peak_frac, double *stats)
{
    return imager_msclean(im, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats,
                          CleanAuto{mask, nsigma, noise, peak_frac, true});
}

int gridhip_imager_msdeconvolve_auto_dev(gridhip_imager *im, const double *vis, double *model, double *image,
                                         int64_t nmajor, int64_t S, const double *scales, const double *bias, double gain,
                                         double threshold, int64_t niter, int64_t border, int64_t patch,
                                         const uint8_t *mask, double nsigma, double peak_frac, double *stats,
                                         double *istats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "msdeconvolve: bad argument");
    GH_CHECK(msclean_check(ctx, im->N, im->psf, image, model, S, scales, bias, gain, threshold, niter, border, patch));
    return deconvolve_auto(im, vis, model, image, nmajor, border, mask, nsigma, peak_frac, istats,
                           [&](int64_t c, const double *noise) {
                               return gridhip_imager_msclean_auto_dev(im, image, model, S, scales, bias, gain, threshold,
                                                                      niter, border, patch, mask, nsigma, noise, peak_frac,
                                                                      stats ? stats + 16 * c : nullptr);
                           });
}

int gridhip_imager_msdeconvolve_dev(gridhip_imager *im, const double *vis, double *model, double *image, int64_t nmajor,
                                    int64_t S, const double *scales, const double *bias, double gain, double threshold,
                                    int64_t niter, int64_t border, int64_t patch, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "msdeconvolve: bad argument");
    GH_CHECK(msclean_check(ctx, im->N, im->psf, image, model, S, scales, bias, gain, threshold, niter, border, patch));
    for (int64_t c = 0; c < nmajor; ++c) {
        GH_CHECK(gridhip_imager_cycle_dev(im, model, vis, image, nullptr));
        GH_CHECK(gridhip_imager_msclean_dev(im, image, model, S, scales, bias, gain, threshold, niter, border, patch,
                                            stats ? stats + 12 * c : nullptr));
    }
    return gridhip_imager_cycle_dev(im, model, vis, image, nullptr);
}

int gridhip_imager_beam_dev(gridhip_imager *im, int64_t window, double cut, double *beam)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(fit_beam_check(ctx, im->N, im->psf, window, cut, beam));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return fit_beam_run(ctx, im->N, im->psf, window, cut, beam);
}

int gridhip_imager_restore_dev(gridhip_imager *im, const double *model, const double *residual, int64_t window, double cut,
                               int64_t support, double *restored, double *beam)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    double placeholder = 0.0;  // (stands for the imager's own block in the checks: it overlaps nothing of the caller's)
    GH_CHECK(fit_beam_check(ctx, im->N, im->psf, window, cut, beam ? beam : &placeholder));
    GH_CHECK(restore_check(ctx, im->N, model, residual, beam ? beam : &placeholder, support, restored));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!beam) {
        if (!im->beam) GH_CHECK(own(im, &im->beam, 64));
        beam = im->beam;
    }
    GH_CHECK(fit_beam_run(ctx, im->N, im->psf, window, cut, beam));
    return restore_run(ctx, im->N, model, residual, beam, support, restored);
}

int gridhip_imager_destroy(gridhip_imager *im)
{
    if (!im) return GRIDHIP_OK;
    (void)hipSetDevice(im->ctx->device);
    (void)hipDeviceSynchronize();
    gridhip_plan_destroy(im->gather);
    gridhip_plan_destroy(im->scatter);
    gridhip_aw_plan_destroy(im->aw_gather);
    gridhip_aw_plan_destroy(im->aw_scatter);
    wstack_release(im->ws_gather);  // (before the transform and the tables they borrow)
    wstack_release(im->ws_scatter);
    fft_plan_drop(im->fft);
    for (void *p : im->owned)
        if (p) (void)hipFree(p);
    delete im;
    return GRIDHIP_OK;
}

int gridhip_imager_automask_dev(gridhip_imager *im, const double *image, uint8_t *mask, int64_t border, int absolute,
                                double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                                double peak_frac, int64_t min_cells, int64_t grow, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    GH_CHECK(automask_check(ctx, im->N, image, mask, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                            min_cells, grow, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!im->am_scratch) GH_CHECK(own(im, &im->am_scratch, automask_scratch_bytes(ctx, im->N)));
    return automask_run(ctx, im->N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                        min_cells, grow, stats, im->am_scratch);
}

int gridhip_imager_find_sources_dev(gridhip_imager *im, const double *image, int64_t border, double thr_hi, double thr_lo,
                                    double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                                    int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps,
                                    double *info, int64_t *count, double *stats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    int64_t N = 0;
    GH_CHECK(sources_check(ctx, im->theta, im->lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                           min_cells, beam, correct, max_c, comps, info, count, stats, &N));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!im->am_scratch) GH_CHECK(own(im, &im->am_scratch, automask_scratch_bytes(ctx, im->N)));
    if (max_c > im->src_rows) {  // (the block it replaces stays the imager's until destruction: earlier calls may be in flight)
        GH_CHECK(own(im, &im->src_scratch, sources_scratch_bytes(im->N, max_c)));
        im->src_rows = max_c;
    }
    return sources_run(ctx, im->N, im->theta, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                       min_cells, beam, correct, max_c, comps, info, count, stats, im->am_scratch, im->src_scratch);
}

// the automask of a deconvolve_automask: what every cycle's mask update takes besides the image, the mask and sigma
struct AutomaskArgs {
    int absolute;
    double thr_hi, thr_lo, nsigma_hi, nsigma_lo, peak_frac;
    int64_t min_cells, grow;
};

// the checks and the loop the two _automask deconvolves share; minor(c, noise): the c-th minor cycle with sigma at `noise`
extern "C++" template <typename Minor>
static int deconvolve_automask(gridhip_imager *im, const double *vis, double *model, double *image, int64_t nmajor,
                               int64_t border, uint8_t *mask, double nsigma, double peak_frac, const AutomaskArgs &am,
                               double *istats, double *astats, Minor minor)
{
    gridhip_ctx *ctx = im->ctx;
    double placeholder = 0.0, none[8];  // (stand for sigma's cell and a stats row in the checks: the loop passes its own)
    if (!mask) return fail(ctx, GRIDHIP_EINVAL, "deconvolve_automask: the mask is the call's state and cannot be NULL");
    GH_CHECK(clean_auto_check(ctx, im->N, image, model, mask, nsigma, &placeholder, peak_frac));
    GH_CHECK(automask_check(ctx, im->N, image, mask, border, am.thr_hi, am.thr_lo, am.nsigma_hi, am.nsigma_lo, &placeholder,
                            am.peak_frac, am.min_cells, am.grow, none));
    if (!istats || !astats) {
        GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
        if (!istats && !im->istats) GH_CHECK(own(im, &im->istats, 64));
        if (!astats && !im->astats) GH_CHECK(own(im, &im->astats, 64));
    }
    for (int64_t c = 0; c < nmajor; ++c) {
        double *ist = istats ? istats + 8 * c : im->istats;
        double *ast = astats ? astats + 8 * c : im->astats;
        GH_CHECK(gridhip_imager_cycle_dev(im, model, vis, image, nullptr));
        GH_CHECK(gridhip_imager_image_stats_dev(im, image, nullptr, border, ist));
        GH_CHECK(gridhip_imager_automask_dev(im, image, mask, border, am.absolute, am.thr_hi, am.thr_lo, am.nsigma_hi,
                                             am.nsigma_lo, (const double *)(ist + 3), am.peak_frac, am.min_cells, am.grow,
                                             ast));
        GH_CHECK(minor(c, (const double *)(ist + 3)));
    }
    return gridhip_imager_cycle_dev(im, model, vis, image, nullptr);
}

int gridhip_imager_deconvolve_automask_dev(gridhip_imager *im, const double *vis, double *model, double *image,
                                           int64_t nmajor, double gain, double threshold, int64_t niter, int64_t border,
                                           int64_t patch, uint8_t *mask, double nsigma, double peak_frac_clean,
                                           int absolute, double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo,
                                           double peak_frac, int64_t min_cells, int64_t grow, double *stats,
                                           double *istats, double *astats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "deconvolve: bad argument");
    GH_CHECK(clean_check(ctx, im->N, im->psf, image, model, gain, threshold, niter, border, patch));
    return deconvolve_automask(im, vis, model, image, nmajor, border, mask, nsigma, peak_frac_clean,
                               AutomaskArgs{absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, peak_frac, min_cells, grow},
                               istats, astats, [&](int64_t c, const double *noise) {
                                   return gridhip_imager_clean_auto_dev(im, image, model, gain, threshold, niter, border,
                                                                        patch, mask, nsigma, noise, peak_frac_clean,
                                                                        stats ? stats + 8 * c : nullptr);
                               });
}

int gridhip_imager_msdeconvolve_automask_dev(gridhip_imager *im, const double *vis, double *model, double *image,
                                             int64_t nmajor, int64_t S, const double *scales, const double *bias,
                                             double gain, double threshold, int64_t niter, int64_t border, int64_t patch,
                                             uint8_t *mask, double nsigma, double peak_frac_clean, int absolute,
                                             double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo,
                                             double peak_frac, int64_t min_cells, int64_t grow, double *stats,
                                             double *istats, double *astats)
{
    if (!im) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = im->ctx;
    if (nmajor < 0 || (im->n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "msdeconvolve: bad argument");
    GH_CHECK(msclean_check(ctx, im->N, im->psf, image, model, S, scales, bias, gain, threshold, niter, border, patch));
    return deconvolve_automask(im, vis, model, image, nmajor, border, mask, nsigma, peak_frac_clean,
                               AutomaskArgs{absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, peak_frac, min_cells, grow},
                               istats, astats, [&](int64_t c, const double *noise) {
                                   return gridhip_imager_msclean_auto_dev(im, image, model, S, scales, bias, gain, threshold,
                                                                          niter, border, patch, mask, nsigma, noise,
                                                                          peak_frac_clean, stats ? stats + 16 * c : nullptr);
                               });
}

}  // extern "C"
